"""fp_pose_color against tests/color_ref.py: EQUAL in every integer field and in the status, zncc equal to the host
formula bit for bit -- the rules are integer coverage, separately rounded f32 and integer sums, so there is no tolerance to choose.  The
cases are those of tests/color_cases.py, which tests/test_color_ref_cpu.py holds to a float64 ray-cast and to hand answers.  Then the
promises of the interface: byte-identical records whatever the batch or the chunking, refusals per record and per call, the untouched
serving path, and neighbours on one model that leave nothing behind."""
import ctypes as C
import os
import re
from unittest import mock

import numpy as np
import pytest

import color_cases as CC
import color_ref as CR
import frame_render_ref as FR
import icp_cases as IC
import test_stage_scratch_gpu as SS
from foundationpose_cpp_amd import FoundationPose, FoundationPoseError, PoseColor, _lib, synthetic as syn
from foundationpose_cpp_amd.api import _p

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "foundationpose_amd.h")).read()
INT_FIELDS = CR.COUNTS + ("status",)


def _const(name):
    return int(re.search(rf"#define {name} (\d+)", HEADER).group(1))


def _raw(m, name, poses, tol=CC.TOL, N=None, out=None):
    """fp_pose_color through the raw ABI -> (return code, records)"""
    e = syn.to_colmajor(np.asarray(poses, np.float32).reshape(-1, 4, 4))
    N = len(e) if N is None else N
    out = (_lib.FpPoseColor * max(N, 1))() if out is None else out
    return m._L.fp_pose_color(m._h, name.encode(), _p(e), N, tol, out), out


def _color(m, name, poses, **kw):
    rc, out = _raw(m, name, poses, **kw)
    m._must(rc)
    return list(out)


def _bytes(rec):
    return b"".join(bytes(r) for r in rec) if isinstance(rec, (list, tuple)) else bytes(rec)


def _equal(what, got, ref):
    """one device record against the reference's dict: every integer, the status, and the bits of zncc"""
    print(f"{what}: device " + " ".join(f"{k}={getattr(got, k)}" for k in INT_FIELDS) + f" sum_mo={list(got.sum_mo)} zncc={float(got.zncc):.6f}")
    for k in INT_FIELDS:
        assert getattr(got, k) == ref[k], (what, k, getattr(got, k), ref[k])
    for k in CR.SUMS:
        assert list(getattr(got, k)) == ref[k], (what, k, list(getattr(got, k)), ref[k])
    assert np.float32(got.zncc).tobytes() == np.float32(ref["zncc"]).tobytes(), (what, got.zncc, ref["zncc"])
    assert got.reserved == 0 and got.reserved_f == 0.0
    status, z = CR.zncc_of(got.n_compared, *(list(getattr(got, k)) for k in CR.SUMS))          # the host formula, from the record's own sums
    if not got.status & (CR.REFUSED_NEAR | CR.REFUSED_RANGE):
        assert got.status == status and np.float32(got.zncc) == np.float32(z)


MESHES = ("batch_47x1", "batch_512", "scene_1", "uv_wrap", "grey", "hand_2x2", "hand_3x2")


@pytest.fixture(scope="module")
def model():
    m = FoundationPose([CC.case(n)["mesh"] for n in MESHES], CC.K)          # geometry-only
    yield m
    m.close()


def _run_case(m, name, **kw):
    c = CC.case(name)
    m.upload_frame(c["rgb"], c["D"])
    if c["colors"] is not None:
        m.set_vertex_colors(c["mesh"].name, c["colors"])
    try:
        return _color(m, c["mesh"].name, c["poses"], **kw)
    finally:
        if c["colors"] is not None:
            m.set_vertex_colors(c["mesh"].name, None)


@pytest.mark.parametrize("name", [n for n in CC.CASES if n != "ragged"])
def test_cases_equal_the_reference(model, name):
    got, ref = _run_case(model, name), CC.expected(name)
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        _equal(f"{name}[{i}]", g, r)
    if name.startswith("scene_"):          # the margin of the true pose over its three equivalents (DESIGN.md section 4.14's table)
        z = sorted((float(g.zncc) for g in got), reverse=True)
        print(f"{name}: zncc of the truth {float(got[0].zncc):.3f}, best of the other equivalents {max(float(g.zncc) for g in got[1:]):.3f}")
        assert CR.resolve(got) == 0 and z[0] == float(got[0].zncc)


def test_the_ragged_frame():
    c = CC.case("ragged")
    m = FoundationPose(c["mesh"], c["K"])
    try:
        m.upload_frame(c["rgb"], c["D"])
        got = _color(m, c["mesh"].name, c["poses"])
        for i, (g, r) in enumerate(zip(got, CC.expected("ragged"))):
            _equal(f"ragged[{i}]", g, r)
        assert got[0].n_model > 500 and c["D"].shape == (80, 96)
    finally:
        m.close()


def test_vertex_colours_and_the_texture_again(model):
    """the colour source is the target's current one: the vertex colours after fp_set_vertex_colors, the texture again after colors == NULL"""
    c = CC.case("vertex_colors")
    name = c["mesh"].name
    model.upload_frame(c["rgb"], c["D"])
    tex = [CR.sums_of_mesh(c["mesh"], P, CC.K, c["rgb"], c["D"], CC.TOL) for P in c["poses"]]
    before = _color(model, name, c["poses"])
    model.set_vertex_colors(name, c["colors"])
    try:
        with_colors = _color(model, name, c["poses"])
    finally:
        model.set_vertex_colors(name, None)
    after = _color(model, name, c["poses"])
    for i in range(len(c["poses"])):
        _equal(f"texture[{i}]", before[i], tex[i])
        _equal(f"vertex colours[{i}]", with_colors[i], CC.expected("vertex_colors")[i])
    assert _bytes(before) == _bytes(after) != _bytes(with_colors)


@pytest.fixture
def tl():
    """the test build (its chunk hooks and launch log) as THE library of the models made inside the test"""
    L = _lib.test_lib()
    for hook in ("fpt_color_set_chunk", "fpt_vsd_set_chunk", "fpt_icp_set_chunk"):
        getattr(L, hook).argtypes = [C.c_int]
        getattr(L, hook).restype = None
    L.fpt_launch_log_arm.argtypes = [C.c_int]
    L.fpt_launch_log_get_all.argtypes = [C.POINTER(C.c_int), C.c_char_p, C.c_int, C.c_int]
    with mock.patch.object(_lib, "lib", _lib.test_lib):
        yield L
    L.fpt_color_set_chunk(0)


def test_a_record_is_the_same_alone_in_any_batch_in_any_chunking_and_again(model, tl):
    c = CC.case("batch_512")
    name, poses = c["mesh"].name, c["poses"]
    model.upload_frame(c["rgb"], c["D"])
    batch = _color(model, name, poses)
    assert len({_bytes(r) for r in batch}) == 7                                      # (the poses do differ)
    assert _bytes(batch) == _bytes(_color(model, name, poses))                        # call to call
    three = _color(model, name, poses[[0, 3, 6]])
    for k, i in enumerate((0, 3, 6)):
        alone = _color(model, name, poses[i:i + 1])
        assert _bytes(alone[0]) == _bytes(batch[i]) == _bytes(three[k]), i
    # forced chunks of 1 and of 3 poses at N = 7, through the test build: the seams change nothing
    m = FoundationPose(c["mesh"], CC.K)
    try:
        m.upload_frame(c["rgb"], c["D"])
        whole = _color(m, name, poses)
        assert _bytes(whole) == _bytes(batch)
        for chunk in (1, 3):
            tl.fpt_color_set_chunk(chunk)
            assert _bytes(_color(m, name, poses)) == _bytes(whole), chunk
        tl.fpt_color_set_chunk(0)
    finally:
        m.close()


def test_refused_poses_are_flagged_per_record(model):
    c = CC.case("refused")
    got = _run_case(model, "refused")
    assert [g.status for g in got] == [0, 1, 0, 2, 0]
    for g in (got[1], got[3]):
        assert g.n_model == 0 and list(g.sum_o) == [0, 0, 0] and g.zncc == 0.0
    clean = _color(model, c["mesh"].name, c["poses"][[0, 2, 4]])
    assert _bytes([got[0], got[2], got[4]]) == _bytes(clean)                          # the neighbours do not notice


def test_the_depth_filter_does_not_reach_the_call():
    c = CC.case("nan_zero_inf")
    m = FoundationPose(c["mesh"], CC.K)
    try:
        m.upload_frame(c["rgb"], c["D"])
        off = _color(m, c["mesh"].name, c["poses"])
        m.set_depth_filter(True)
        on = _color(m, c["mesh"].name, c["poses"])
        m.upload_frame(c["rgb"], c["D"])
        again = _color(m, c["mesh"].name, c["poses"])
        assert _bytes(off) == _bytes(on) == _bytes(again)
        _equal("depth filter on", on[0], CC.expected("nan_zero_inf")[0])
    finally:
        m.close()


def test_refusals_leave_out_untouched():
    c = CC.case("batch_512")
    G = c["poses"][0]
    max_batch, cap = _const("FP_MAX_BATCH"), int(re.search(r"#define FP_COLOR_MAX_WORK (\d+)LL", HEADER).group(1))
    # the work cap: every pose so near that its bound is the whole 1920 x 1080 frame (2040 tiles), a mesh of F degenerate faces
    tiles = 60 * 34
    F = cap // (max_batch * tiles) + 1
    base = c["mesh"]
    many = syn.Mesh("many", base.vertices, base.normals, base.texcoords, np.zeros((F, 3), np.int32), base.texture).finalize()
    near = IC.pose(CC._rot_y(90.0), (0.0, 0.0, 0.09))          # the bounding sphere reaches the camera plane, no vertex does
    m = FoundationPose([base, many], CC.K)
    skew = np.array(CC.K, np.float32)
    skew[0, 1] = 0.5
    ms = FoundationPose(base, skew)
    try:
        def refused(match, *a, model=m, **kw):
            n = max(kw.get("N") or 1, len(np.asarray(a[1]).reshape(-1, 4, 4)))
            out = (_lib.FpPoseColor * n)()
            C.memset(out, 0x5A, C.sizeof(out))
            before = _bytes(out)
            rc, _ = _raw(model, *a, out=out, **kw)
            assert rc != 0 and re.search(match, _lib.last_error()), (match, rc, _lib.last_error())
            assert _bytes(out) == before

        refused("no frame uploaded", base.name, [G])
        m.upload_frame(c["rgb"], c["D"])
        ms.upload_frame(c["rgb"], c["D"])
        assert _raw(m, base.name, [G])[0] == 0
        refused(r"fp_pose_color: the model's K is not a plain pinhole matrix: K\[1\]", base.name, [G], model=ms)
        refused("unknown target_name", "nobody", [G])
        refused(r"1\.\.FP_MAX_BATCH", base.name, [G], N=0)
        refused(r"1\.\.FP_MAX_BATCH", base.name, [G] * (max_batch + 1))
        for value in (float("nan"), float("inf"), -0.01):
            refused("tol_m", base.name, [G], tol=value)
        assert _raw(m, base.name, [G], tol=0.0)[0] == 0
        for value in (float("nan"), float("inf"), -float("inf")):
            for where in ((0, 0), (2, 3), (3, 3)):
                bad = np.array(G)
                bad[where] = value
                refused(r"non-finite.*poses\[1\]", base.name, [G, bad])
        # the cap: FP_MAX_BATCH poses over the whole of a large frame are one face too many; nothing is launched
        m.upload_frame(np.zeros((1080, 1920, 3), np.uint8), np.zeros((1080, 1920), np.float32))
        assert max_batch * tiles * F > cap >= max_batch * tiles * (F - 1)
        refused("FP_COLOR_MAX_WORK", "many", [near] * max_batch)
        rc, out = _raw(m, "many", [near])
        assert rc == 0 and out[0].n_model == 0 and out[0].status == CR.TOO_FEW
    finally:
        m.close()
        ms.close()


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
    """a Register followed by a Track after the two calls equals one before them, bit for bit and launch for launch; a Track from a host
    frame leaves only its crop window, and a submitted Track is pending: both refuse the calls"""
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
        m.upload_frame(syn_scene.rgb, syn_scene.depth)   # (as before the calls below: both logged rounds follow an upload)
        (_, pose), log_before = _logged(tl, serve)
        out = (_lib.FpPoseColor * 1)()
        C.memset(out, 0x5A, C.sizeof(out))
        rc, _ = _raw(m, syn_mesh.name, [pose], out=out)
        assert rc != 0 and "only its crop window" in _lib.last_error() and _bytes(out) == b"\x5a" * C.sizeof(out)
        m.upload_frame(syn_scene.rgb, syn_scene.depth)
        G = syn_scene.gt_pose
        recs = m.pose_color(syn_mesh.name, [pose, G])
        ref = [CR.sums_of_mesh(syn_mesh, P, syn_scene.K, syn_scene.rgb, syn_scene.depth, 0.005) for P in (pose, G)]
        for got, r in zip(recs, ref):
            assert isinstance(got, PoseColor) and [getattr(got, k) for k in INT_FIELDS] == [r[k] for k in INT_FIELDS]
            assert all(list(getattr(got, k)) == r[k] for k in CR.SUMS) and np.float32(got.zncc) == r["zncc"]
        assert recs[1].n_compared > 1000 and recs[1].zncc > 0.5
        flip = np.array(G, np.float32)
        flip[:3, :3] = G[:3, :3] @ np.diag([-1.0, -1.0, 1.0]).astype(np.float32)
        sym = np.eye(4, dtype=np.float32)
        sym[:3, :3] = np.diag([-1.0, -1.0, 1.0])
        c = np.asarray(syn_mesh.center, np.float32)
        sym[:3, 3] = c - sym[:3, :3] @ c
        back, best, all_recs = m.resolve_symmetry(syn_mesh.name, flip, [sym])
        print(f"640 x 480 scene: zncc of the flipped pose {all_recs[0].zncc:.3f}, of its equivalent {all_recs[1].zncc:.3f}")
        assert best == 1 and np.abs(back - G).max() < 1e-6
        after, log_after = _logged(tl, serve)
        assert after[0] == before[0][0] and log_after == log_before
        hyp = syn.to_colmajor(syn.perturb_pose(syn_scene.gt_pose))
        m._must(m._L.fp_track_submit(m._h, _p(syn_scene.rgb), _p(syn_scene.depth), 0, hw[0], hw[1], _p(hyp), syn_mesh.name.encode(), 1))
        rc, _ = _raw(m, syn_mesh.name, [pose], out=out)
        assert rc != 0 and "has not been waited for" in _lib.last_error() and _bytes(out) == b"\x5a" * C.sizeof(out)
        with pytest.raises(FoundationPoseError, match="has not been waited for"):
            m.resolve_symmetry(syn_mesh.name, flip, [sym])
        m._must(m._L.fp_track_wait(m._h, _p(np.zeros(16, np.float32))))
        # the profiler's families
        m.upload_frame(syn_scene.rgb, syn_scene.depth)
        m.profile_reset(); m.profile(True)
        m.pose_color(syn_mesh.name, [pose])
        rep = m.profile_report()
        m.profile(False)
        assert rep["color_vertex"]["calls"] == 1 and rep["color_tile"]["calls"] == 1
    finally:
        m.close()


def test_neighbours_on_one_model_leave_nothing_behind(tl):
    """in the spirit of tests/test_stage_scratch_gpu.py (its window, its poses): fp_pose_vsd, fp_pose_color, fp_refine_depth and
    fp_pose_color again on ONE model each equal the same call on a fresh model"""
    small, large = syn.make_mesh(1, textured=True, name="ico1t"), CC.mesh3()

    def fresh():
        m = FoundationPose([small, large], SS.K)
        m.upload_frame(SS.RGB, SS.DEPTH)
        return m

    steps = [("pose_vsd, small mesh, chunks of 1", {"fpt_vsd_set_chunk": 1}, lambda m: SS._vsd(m, small.name, SS.EST, SS.GTS)),
             ("pose_color, large mesh, chunks of 2", {"fpt_color_set_chunk": 2}, lambda m: _bytes(_color(m, large.name, SS.EST))),
             ("refine_depth, small mesh, chunks of 2", {"fpt_icp_set_chunk": 2}, lambda m: SS._refine(m, small.name, SS.EST, 2)),
             ("pose_color, small mesh", {}, lambda m: _bytes(_color(m, small.name, SS.EST[:2])))]
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
    first = _lib.FpPoseColor.from_buffer_copy(got[1][:C.sizeof(_lib.FpPoseColor)])
    _equal("pose_color on the shared model", first, CR.sums_of_mesh(large, SS.EST[0], SS.K, SS.RGB, SS.DEPTH, CC.TOL))


def test_through_the_python_interface(model):
    c = CC.case("batch_47x1")
    model.upload_frame(c["rgb"], c["D"])
    recs = model.pose_color(c["mesh"].name, c["poses"])
    raw = _color(model, c["mesh"].name, c["poses"])
    assert len(recs) == 7 and all(isinstance(r, PoseColor) for r in recs)
    for r, w in zip(recs, raw):
        assert [getattr(r, k) for k in INT_FIELDS] == [getattr(w, k) for k in INT_FIELDS]
        assert all(getattr(r, k) == tuple(getattr(w, k)) for k in CR.SUMS) and r.zncc == float(w.zncc)
    assert np.float32(recs[0].zncc) == CC.expected("batch_47x1")[0]["zncc"] > 0.5 and recs[5].status == CR.TOO_FEW          # 2 degrees off; wholly outside
    with pytest.raises(FoundationPoseError, match="unknown target_name"):
        model.pose_color("nobody", c["poses"])
