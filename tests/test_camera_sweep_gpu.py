"""The frame-resolution pose calls on the device under a GENERAL camera: fx != fy by 10 % and more, a principal
point off the centre and off the pixel grid, landscape, portrait and odd frames.  The cases are those of tests/camera_cases.py, whose
references tests/test_camera_cases_cpu.py holds to float64 -- and to cameras broken on purpose -- before a kernel sees them.  K is fixed
at creation, so there is one geometry-only model per case; every test uploads the case's frame and goes through the raw ABI.  Then what
K these calls accept: a matrix that is not a plain pinhole is refused by the seven calls that read fx, fy, cx, cy only, and still serves
Register and Track."""
import ctypes as C
import functools
import re
from unittest import mock

import numpy as np
import pytest

import camera_cases as CC
import frame_render_ref as FR
import icp_ref as IR
import pose_error_ref as PR
import scene_render_ref as SRR
import search_ref as SR
import vsd_ref as VR
from foundationpose_cpp_amd import FoundationPose, _lib, synthetic as syn
from foundationpose_cpp_amd.api import FP_HOST, _p
from test_register_depth_gpu import _composed, _register

pytestmark = pytest.mark.gpu

NORMALIZED, ADDS = 1, 1
VSD_TAUS = (0.05, 0.2, 0.5)
SEARCH_STEPS, SEARCH_TOL = 5, 0.05


def _col(poses):
    return syn.to_colmajor(np.asarray(poses, np.float32).reshape(-1, 4, 4))


def _search(m, name, poses, step_m, tol_m, vertex_step, n_steps=SEARCH_STEPS, out=None):
    e = _col(poses)
    out = (_lib.FpPoseSearch * len(e))() if out is None else out
    return m._L.fp_pose_search(m._h, name.encode(), _p(e), len(e), n_steps, step_m, tol_m, vertex_step, out), out


def _refine(m, name, poses, iterations, gate, out_p=None, out=None):
    e = _col(poses)
    out_p = np.zeros((len(e), 16), np.float32) if out_p is None else out_p
    out = (_lib.FpDepthRefine * len(e))() if out is None else out
    return m._L.fp_refine_depth(m._h, name.encode(), _p(e), len(e), iterations, gate, 0, _p(out_p), out), syn.from_colmajor(out_p), out


def _vsd(m, name, est, gt, delta, taus=VSD_TAUS, out=None):
    e, g = _col(est), _col(gt)
    t = np.ascontiguousarray(np.asarray(taus, np.float32))
    out = (_lib.FpPoseVsd * len(e))() if out is None else out
    return m._L.fp_pose_vsd(m._h, name.encode(), _p(e), len(e), _p(g), len(g), delta, _p(t), len(t), NORMALIZED, out), out


def _errors(m, name, est, gt, sym, step, out=None):
    e, g, s = _col(est), _col(gt), _col(sym)
    out = (_lib.FpPoseError * len(e))() if out is None else out
    return m._L.fp_pose_errors(m._h, name.encode(), _p(e), len(e), _p(g), len(g), _p(s), len(s), step, ADDS, out), out


def _scene(m, names, poses, hw, records=True, planes=None):
    spec = FoundationPose.SCENE_OUTPUTS
    planes = {n: np.full(tuple(hw) + spec[n][1], 77, spec[n][0]) for n in SRR.OUTPUTS} if planes is None else planes
    rec = _lib.FpSceneRender(**{n: _p(a) for n, a in planes.items()})
    recs = (_lib.FpSceneObject * len(names))()
    C.memset(recs, 0x5A, C.sizeof(recs))
    rc = m._L.fp_render_scene(m._h, len(names), (C.c_char_p * len(names))(*[n.encode() for n in names]), _p(_col(poses)), 0.005, C.byref(rec),
                              recs if records else None, FP_HOST)
    return rc, planes, recs


def _bytes(recs):
    return b"".join(bytes(r) for r in recs)


def _ok(m, rc):
    assert rc == 0, _lib.last_error()


@pytest.fixture(scope="module")
def model_of():
    """one geometry-only model (NULL weights) per case, made when first asked for, with the case's frame uploaded"""
    made = {}

    def get(seed):
        if seed not in made:
            c = CC.camera_case(seed)
            made[seed] = FoundationPose([c.mesh, c.convex], c.K)
        made[seed].upload_frame(CC.camera_case(seed).rgb, CC.camera_case(seed).depth)
        return made[seed]

    yield get
    for m in made.values():
        m.close()


# ---- fp_pose_search ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vertex_step", [1, 3])
@pytest.mark.parametrize("seed", CC.SEEDS)
def test_pose_search_equals_the_restatement(model_of, seed, vertex_step):
    c, m = CC.camera_case(seed), model_of(seed)
    poses = np.concatenate([c.E, c.G])
    step, tol = np.float32(c.mesh.diameter) / np.float32(16), SEARCH_TOL * c.mesh.diameter
    ref = SR.records(FR.centred(c.mesh), SR.normals_of(c.mesh), poses, c.K, c.depth, SEARCH_STEPS, step, tol, vertex_step)
    rc, got = _search(m, c.mesh.name, poses, float(step), tol, vertex_step)
    _ok(m, rc)
    for i, (g, r) in enumerate(zip(got, ref)):
        print(f"seed {seed} step {vertex_step} pose {i}: " + " ".join(f"{k}={getattr(g, k)}" for k in SR.FIELDS))
        assert {k: getattr(g, k) for k in SR.FIELDS} == r, (seed, vertex_step, i)
    assert ref[4]["n_inlier"] > ref[4]["n_facing"] // 2 and ref[4]["status"] == 0          # the truth of the frame's own rendering


# ---- fp_refine_depth --------------------------------------------------------------------------------------------------------------------
def _same_as_sums(rec, ref, what):
    assert [getattr(rec, k) for k in IR.COUNTS] == [ref[k] for k in IR.COUNTS], (what, [getattr(rec, k) for k in IR.COUNTS], [ref[k] for k in IR.COUNTS])
    assert list(rec.sums_q32) == ref["sums"], what


@pytest.mark.parametrize("seed", CC.SEEDS)
def test_refine_depth_one_evaluation_equals_the_restatement(model_of, seed):
    c, m = CC.camera_case(seed), model_of(seed)
    poses = np.concatenate([c.E, c.G])
    rc, out_p, recs = _refine(m, c.mesh.name, poses, 0, c.gate)
    _ok(m, rc)
    assert out_p.tobytes() == poses.tobytes()
    v = FR.centred(c.mesh)
    for i, r in enumerate(recs):
        ref = IR.sums(v, c.mesh.faces, poses[i], c.K, c.depth, c.gate, c.mesh.diameter)
        print(f"seed {seed} pose {i}: " + " ".join(f"{k}={getattr(r, k)}" for k in IR.COUNTS))
        _same_as_sums(r, ref, (seed, i))
        assert r.status == 0 and r.n_model >= 400
    assert recs[4].n_used > 300 and recs[4].n_model - recs[4].n_valid >= 12          # the holes on the object are not valid


@functools.lru_cache(maxsize=None)
def _refined64(seed):
    c = CC.camera_case(seed)
    return IR.icp64(c.mesh, c.E[0], c.K, c.depth, c.gate, CC.ICP_ITERATIONS)["pose"]


@pytest.mark.parametrize("seed", CC.SEEDS)
def test_refine_depth_ends_where_float64_ends(model_of, seed):
    c, m = CC.camera_case(seed), model_of(seed)
    rc, P, recs = _refine(m, c.mesh.name, c.E, CC.ICP_ITERATIONS, c.gate)
    _ok(m, rc)
    deg, dist = IR.pose_gap(P[0], _refined64(seed))
    gdeg, gdist = IR.pose_gap(P[0], c.G[0])
    print(f"seed {seed}: against (b) {deg:.4f} deg {dist * 1e3:.4f} mm (bound {CC.AB_BOUND_DEG:.4f} / {CC.AB_BOUND_M * 1e3:.4f}); against the truth "
          f"{gdeg:.4f} deg {gdist * 1e3:.4f} mm (bound {CC.GT_BOUND_DEG:.4f} / {CC.GT_BOUND_M * 1e3:.4f}); {recs[0].iterations} iterations, n_used {recs[0].n_used}")
    assert deg <= CC.AB_BOUND_DEG and dist <= CC.AB_BOUND_M
    assert gdeg <= CC.GT_BOUND_DEG and gdist <= CC.GT_BOUND_M
    assert recs[0].rank == 6 and recs[0].n_used > 300
    v = FR.centred(c.mesh)
    for i in range(len(c.E)):                       # the record describes the returned pose, on every one of the four
        if not recs[i].status & (IR.REFUSED_NEAR | IR.REFUSED_RANGE):
            _same_as_sums(recs[i], IR.sums(v, c.mesh.faces, P[i], c.K, c.depth, c.gate, c.mesh.diameter), (seed, i))
    rc, P1, recs1 = _refine(m, c.mesh.name, c.E[:1], CC.ICP_ITERATIONS, c.gate)          # alone
    _ok(m, rc)
    assert P1[0].tobytes() == P[0].tobytes() and bytes(recs1[0]) == bytes(recs[0])


# ---- fp_pose_vsd ------------------------------------------------------------------------------------------------------------------------
def _vsd_equal(what, got, ref):
    for k in VR.COUNTS + ("status",):
        assert getattr(got, k) == ref[k], (what, k, getattr(got, k), ref[k])
    assert list(got.n_fail) == ref["n_fail"], (what, list(got.n_fail), ref["n_fail"])
    assert np.array(list(got.vsd), np.float32).tobytes() == np.array(ref["vsd"], np.float32).tobytes(), what


@pytest.mark.parametrize("which", ["dented", "convex"])
@pytest.mark.parametrize("seed", CC.SEEDS)
def test_pose_vsd_equals_the_restatement(model_of, seed, which):
    c, m = CC.camera_case(seed), model_of(seed)
    mesh = c.mesh if which == "dented" else c.convex
    delta = 0.15 * mesh.diameter
    for gt in (c.G, c.G[:1]):                       # paired truths, then every estimate against the one truth the frame shows
        rc, got = _vsd(m, mesh.name, c.E, gt, delta)
        _ok(m, rc)
        ref = VR.vsd(mesh, c.E, gt, c.depth, c.K, delta, VSD_TAUS)
        for i, (g, r) in enumerate(zip(got, ref)):
            print(f"seed {seed} {which} n_gt {len(gt)} pose {i}: " + " ".join(f"{k}={getattr(g, k)}" for k in VR.COUNTS) + f" n_fail={list(g.n_fail)[:3]}")
            _vsd_equal((seed, which, len(gt), i), g, r)
        if which == "convex" and len(gt) > 1:       # ... and the convex mesh inside the float64 intervals
            for i, g in enumerate(got):
                iv, n_unsure = VR.intervals(mesh, c.E[i], c.G[i], c.depth, c.K, delta, VSD_TAUS)
                rec = dict({k: getattr(g, k) for k in VR.COUNTS}, n_fail=list(g.n_fail))
                assert VR.inside(rec, iv) == [] and n_unsure <= rec["n_union"] / 3, (seed, i, n_unsure)
    assert 0 < got[0].n_inter < got[0].n_union


# ---- fp_pose_errors ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vertex_step", [1, 3])
@pytest.mark.parametrize("seed", CC.SEEDS)
def test_pose_errors_against_float64(model_of, seed, vertex_step):
    """the allowances are those pose_error_ref derives and tests/test_pose_error_gpu.py applies; MSPD is the field that reads K"""
    c, m = CC.camera_case(seed), model_of(seed)
    sym = CC.symmetries(c.mesh)
    ref = PR.pose_errors(FR.centred(c.mesh), c.mesh.center, c.K, c.E, c.G, sym, vertex_step)
    rc, got = _errors(m, c.mesh.name, c.E, c.G, sym, vertex_step)
    _ok(m, rc)
    for i, (g, r) in enumerate(zip(got, ref)):
        bound = PR.pixel_bound(r, c.K, r["mspd_px"])
        print(f"seed {seed} step {vertex_step} pose {i}: mspd_px device {g.mspd_px:.9g} reference {r['mspd_px']:.9g} bound {bound:.3g}; " +
              "; ".join(f"{f} {getattr(g, f):.9g} / {r[f]:.9g} / {PR.metric_bound(r, r[f]):.3g}" for f in ("add_m", "adds_m", "mssd_m")))
        for f in ("add_m", "adds_m", "mssd_m"):
            assert abs(getattr(g, f) - r[f]) <= PR.metric_bound(r, r[f]), (seed, i, f, getattr(g, f), r[f])
        assert g.n_vertices == r["n_vertices"] and r["best_sym_mspd"] >= 0
        assert abs(g.mspd_px - r["mspd_px"]) <= bound, (seed, i, g.mspd_px, r["mspd_px"], bound)
        assert r["per_sym_mspd"][g.best_sym_mspd] - r["mspd_px"] <= 2 * bound and r["per_sym_mssd"][g.best_sym] - r["mssd_m"] <= 2 * PR.metric_bound(r, r["mssd_m"])
        if np.sort(r["per_sym_mspd"])[1] - r["mspd_px"] > 1.0:
            assert g.best_sym_mspd == r["best_sym_mspd"]
        if np.sort(r["per_sym_mssd"])[1] - r["mssd_m"] > 1e-3:
            assert g.best_sym == r["best_sym"]
            assert abs(g.rot_deg - r["rot_deg"]) <= PR.angle_bound(r["rot_deg"]) and abs(g.trans_m - r["trans_m"]) <= PR.length_bound(r["trans_m"])


# ---- fp_render_scene --------------------------------------------------------------------------------------------------------------------
def _planes_equal(what, got, ref):
    for n in got:
        g, r = (got[n].view(np.uint32), ref[n].view(np.uint32)) if n == "model_depth" else (got[n], ref[n])
        bad = g != r
        assert not bad.any(), f"{what}: {n} differs at {int(bad.sum())} of {bad.size} entries, first at {tuple(int(i) for i in np.argwhere(bad)[0])}"


@pytest.mark.parametrize("seed", CC.SEEDS)
def test_render_scene_equals_the_restatement(model_of, seed):
    c, m = CC.camera_case(seed), model_of(seed)
    names = [c.mesh.name, c.convex.name, c.mesh.name]          # one mesh twice; the convex one interpenetrates the first
    poses = [c.G[0], c.E[0], c.G[1]]
    meshes = {c.mesh.name: c.mesh, c.convex.name: c.convex}
    ref, ref_rec = SRR.render([(FR.centred(meshes[n]), meshes[n].faces, P) for n, P in zip(names, poses)], c.K, c.rgb, c.depth)
    rc, got, recs = _scene(m, names, poses, (c.H, c.W))
    _ok(m, rc)
    _planes_equal(f"seed {seed}", got, ref)
    table = np.array([[getattr(r, f) for f in SRR.RECORD] for r in recs], np.int64)
    print(f"seed {seed}: records\n{table}")
    assert np.array_equal(table, ref_rec) and (table[:, 0] >= 400).all() and table[:2, 2].sum() > 0          # (the first two hide parts of each other)
    # one object: fp_render_pose's planes
    for P in (c.G[0], c.G[3]):
        one = m.render_pose(c.mesh.name, P)
        rc, got, recs = _scene(m, [c.mesh.name], [P], (c.H, c.W))
        _ok(m, rc)
        _planes_equal(f"seed {seed}, one object", {n: got[n] for n in ("model_depth", "visible_mask", "tri_id", "overlay")}, one)
        assert np.array_equal(got["instance_id"] * 255, one["model_mask"]) and np.array_equal(got["cover_bits"], (one["model_mask"] > 0).astype(np.uint64))
        want = FR.render(FR.centred(c.mesh), c.mesh.faces, P, c.K, c.rgb, c.depth)
        _planes_equal(f"seed {seed}, fp_render_pose", one, want)


# ---- fp_register_depth ------------------------------------------------------------------------------------------------------------------
def test_register_depth_equals_the_composition_and_reaches_the_truth(model_of):
    seed = CC.REGISTER_SEED
    c, m = CC.camera_case(seed), model_of(seed)
    rgb, D, mask, G = CC.register_scene()
    rc, pose, rec = _register(m, c.mesh.name, rgb, D, mask, 16, 0.005, 15)
    assert rc == 0, _lib.last_error()
    want_pose, want_rec, hyp = _composed(m, c.mesh, c.mesh.name, rgb, D, mask, 16, 0.005, 15)
    assert pose.tobytes() == want_pose.tobytes() and bytes(rec) == bytes(want_rec)
    assert (rec.n_hypotheses, rec.n_candidates) == (252, 16) and rec.rank_key == rec.refine.n_used - rec.refine.n_behind > 0
    got = CC.mssd(c.mesh, pose, G)
    print(f"hypothesis {rec.hypothesis} (step {rec.search.best_step}, score {rec.search.score}), rank_key {rec.rank_key}, MSSD {got * 1e3:.3f} mm "
          f"(float64 reference {CC.REF_MSSD_MM:.3f} mm, bound {CC.REGISTER_BOUND_M * 1e3:.3f} mm)")
    assert got <= CC.REGISTER_BOUND_M


# ---- the tile bound under this camera: forcing one pose per chunk changes nothing -------------------------------------------------------
@pytest.fixture
def tl():
    """the test build (its chunk hooks) as THE library of the models made inside the test"""
    L = _lib.test_lib()
    for hook in (L.fpt_vsd_set_chunk, L.fpt_icp_set_chunk):
        hook.argtypes = [C.c_int]
        hook.restype = None
    with mock.patch.object(_lib, "lib", _lib.test_lib):
        yield L
    L.fpt_vsd_set_chunk(0)
    L.fpt_icp_set_chunk(0)


@pytest.mark.parametrize("seed", CC.SEEDS)
def test_one_pose_per_chunk_changes_nothing(tl, seed):
    c = CC.camera_case(seed)
    est = np.stack([c.E[3], c.G[3], c.E[0], c.E[1], c.E[2]])          # the near pose first: it covers the most tiles
    delta = 0.15 * c.mesh.diameter
    m = FoundationPose([c.mesh, c.convex], c.K)
    try:
        m.upload_frame(c.rgb, c.depths[3])
        results = []
        for chunk in (0, 1):
            tl.fpt_vsd_set_chunk(chunk)
            tl.fpt_icp_set_chunk(chunk)
            rc, paired = _vsd(m, c.mesh.name, est, np.stack([c.G[3], c.G[3], c.G[0], c.G[1], c.G[2]]), delta)
            _ok(m, rc)
            rc, single = _vsd(m, c.mesh.name, est, c.G[3:], delta)
            _ok(m, rc)
            rc, P, recs = _refine(m, c.mesh.name, est, 3, c.gate)
            _ok(m, rc)
            results.append((_bytes(paired), _bytes(single), P.tobytes(), _bytes(recs)))
        assert results[0] == results[1]
        ref = VR.vsd(c.mesh, est[:2], c.G[3:], c.depths[3], c.K, delta, VSD_TAUS)
        _vsd_equal((seed, "near"), single[0], ref[0])
        assert single[1].n_inter == single[1].n_union == ref[1]["n_union"] > 1000
    finally:
        m.close()


# ---- what K the frame calls accept ------------------------------------------------------------------------------------------------------
def _not_pinhole(K, entry, value):
    K = np.array(K, np.float32)
    K.ravel()[entry] = value
    return K


@pytest.mark.parametrize("entry,value", [(1, 0.5), (3, -0.25), (6, 1e-4), (7, 1e-4), (8, 1.001), (0, -120.0), (4, float("nan")), (4, 0.0)])
def test_a_matrix_that_is_not_a_plain_pinhole_is_refused(entry, value):
    """on the host, before anything is launched (no frame is uploaded, and the message is the camera's, not "no frame uploaded"); the
    message names the entry; the outputs keep their 0x5A"""
    c = CC.camera_case(0)
    m = FoundationPose([c.mesh, c.convex], _not_pinhole(c.K, entry, value))
    try:
        name, G = c.mesh.name, c.G[:2]
        match = rf"fp_\w+: the model's K is not a plain pinhole matrix: K\[{entry}\]"

        def filled(kind, n):
            out = (kind * n)()
            C.memset(out, 0x5A, C.sizeof(out))
            return out

        def refused(rc, call, *outs):
            assert rc != 0 and re.search(match, _lib.last_error()) and call in _lib.last_error(), (call, rc, _lib.last_error())
            for o in outs:
                assert (bytes(o) if not isinstance(o, np.ndarray) else o.tobytes()) == b"\x5a" * (C.sizeof(o) if not isinstance(o, np.ndarray) else o.nbytes), call

        for uploaded in (False, True):
            if uploaded:
                m.upload_frame(c.rgb, c.depth)
            out = filled(_lib.FpPoseSearch, 2)
            refused(_search(m, name, G, 0.01, 0.005, 1, out=out)[0], "fp_pose_search", out)
            out, out_p = filled(_lib.FpDepthRefine, 2), np.full((2, 16), np.frombuffer(b"\x5a" * 4, np.float32)[0], np.float32)
            refused(_refine(m, name, G, 2, c.gate, out_p=out_p, out=out)[0], "fp_refine_depth", out, out_p)
            out = filled(_lib.FpPoseVsd, 2)
            refused(_vsd(m, name, G, G, 0.01, out=out)[0], "fp_pose_vsd", out)
            out = filled(_lib.FpPoseError, 2)
            refused(_errors(m, name, G, G, CC.symmetries(c.mesh), 1, out=out)[0], "fp_pose_errors", out)
            spec = FoundationPose.SCENE_OUTPUTS
            planes = {n: np.frombuffer(b"\x5a" * (c.H * c.W * int(np.prod(spec[n][1] or (1,))) * np.dtype(spec[n][0]).itemsize), spec[n][0]).copy() for n in SRR.OUTPUTS}
            rc, planes, recs = _scene(m, [name, name], G, (c.H, c.W), planes=planes)
            refused(rc, "fp_render_scene", recs, *planes.values())
            depth = np.frombuffer(b"\x5a" * (c.H * c.W * 4), np.float32).copy()
            rc = m._L.fp_render_pose(m._h, name.encode(), _p(_col(G[:1])), 0.005, C.byref(_lib.FpFrameRender(model_depth=_p(depth))), FP_HOST)
            refused(rc, "fp_render_pose", depth)
            out_pose, rec = np.frombuffer(b"\x5a" * 64, np.float32).copy(), _lib.FpDepthRegister()
            C.memset(C.byref(rec), 0x5A, C.sizeof(rec))
            rgb, D, mask, _ = CC.register_scene(0)
            rc, _, _ = _register(m, name, rgb, D, mask, out=out_pose, rec=rec)
            refused(rc, "fp_register_depth", out_pose, rec)
    finally:
        m.close()


def test_a_general_matrix_still_registers_and_tracks(disc_nets, syn_mesh, syn_scene):
    """fp_create, Register and Track take all nine entries, as the reference does: with a skew the crop path runs and a frame call says
    why it does not"""
    K = _not_pinhole(syn_scene.K, 1, 0.75)
    m = FoundationPose(syn_mesh, K, disc_nets[0], disc_nets[1])
    try:
        m.set_inplane_steps(1)
        ok, reg = m.Register(syn_scene.rgb, syn_scene.depth, syn_scene.mask, syn_mesh.name)
        assert ok and np.isfinite(reg).all(), m.last_error
        ok, trk = m.Track(syn_scene.rgb, syn_scene.depth, reg, syn_mesh.name)
        assert ok and np.isfinite(trk).all(), m.last_error
        plain = FoundationPose(syn_mesh, syn_scene.K, disc_nets[0], disc_nets[1])
        try:
            plain.set_inplane_steps(1)
            ok, reg0 = plain.Register(syn_scene.rgb, syn_scene.depth, syn_scene.mask, syn_mesh.name)
            assert ok and reg0.tobytes() != reg.tobytes()          # the skew does reach the crop path
        finally:
            plain.close()
        m.upload_frame(syn_scene.rgb, syn_scene.depth)
        out = (_lib.FpPoseSearch * 1)()
        C.memset(out, 0x5A, C.sizeof(out))
        rc, _ = _search(m, syn_mesh.name, [reg], 0.01, 0.005, 3, out=out)
        assert rc != 0 and re.search(r"K\[1\].*Register and Track take a general K", _lib.last_error()) and bytes(out) == b"\x5a" * C.sizeof(out)
    finally:
        m.close()
