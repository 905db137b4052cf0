"""fp_render_pose against tests/frame_render_ref.py: EQUAL on model_mask, visible_mask, tri_id, model_depth (bit
pattern) and overlay -- the rules are integer coverage and separately rounded f32, so there is no tolerance to choose.  The cases are
the smallest that can break the kernels: frames that cut the 32-px tiles on both axes, objects partly outside the frame, triangles
larger and much smaller than a tile, a box whose triangles span many tile seams, duplicated and degenerate faces; then the plumbing:
device outputs into a re-Register, subsets of outputs, the untouched serving path, the refusals."""
import ctypes as C
from unittest import mock

import numpy as np
import pytest
import torch

import frame_render_ref as FR
import geometry_cases as GC
from foundationpose_cpp_amd import FoundationPose, FoundationPoseError, _lib, synthetic as syn
from foundationpose_cpp_amd.api import FP_DEVICE, FP_HOST, _p

pytestmark = pytest.mark.gpu

TILE = 32
# one seed per frame size of geometry_cases.SWEEP_SIZES (size = seed % 6, subdivisions = 1 + seed % 3): 0, 1 and 3 are the first seeds of
# their size; 32, 10 and 17 the first of theirs at which the reference's own near check refuses one of the 0.12 m poses
SEEDS = [0, 1, 32, 3, 10, 17]


def _render(m, name, pose, hw, tol_m=0.005, want=FR.OUTPUTS):
    """fp_render_pose with host outputs through the raw ABI (the frame size is the caller's business here, as it is in C)"""
    spec = FoundationPose.RENDER_OUTPUTS
    out = {n: np.full(tuple(hw) + spec[n][1], 77, spec[n][0]) for n in want}       # (pre-filled: every pixel must be WRITTEN)
    rec = _lib.FpFrameRender(**{n: _p(a) for n, a in out.items()})
    p16 = syn.to_colmajor(np.asarray(pose, np.float32).reshape(4, 4))
    m._must(m._L.fp_render_pose(m._h, name.encode(), _p(p16), tol_m, C.byref(rec), FP_HOST))
    return out


def _same(what, got, ref):
    for n in got:
        g, r = got[n], ref[n]
        if n == "model_depth":
            g, r = g.view(np.uint32), r.view(np.uint32)
        bad = g != r
        assert not bad.any(), f"{what}: {n} differs at {int(bad.sum())} of {bad.size} entries, first at {tuple(int(i) for i in np.argwhere(bad)[0])}"


@pytest.mark.parametrize("seed", SEEDS)
def test_random_cases_equal_the_reference(seed):
    mesh, K, rgb, depth, poses, (H, W) = GC.random_case(seed)
    assert (W, H) == GC.SWEEP_SIZES[SEEDS.index(seed)]
    v = FR.centred(mesh)
    m = FoundationPose(mesh, K)                     # geometry-only
    try:
        m.upload_frame(rgb, depth)
        drawn = refused = 0
        for i, pose in enumerate(poses):
            why = FR.refused(v, pose, K)
            if why:                                 # no clipper: an error, not a picture
                with pytest.raises(FoundationPoseError, match="pose refused"):
                    _render(m, mesh.name, pose, (H, W))
                refused += 1
                continue
            ref = FR.render(v, mesh.faces, pose, K, rgb, depth)
            _same(f"seed {seed} pose {i}", _render(m, mesh.name, pose, (H, W)), ref)
            drawn += int(ref["model_mask"].any())
        assert drawn >= 3 and refused == {32: 2, 10: 2, 17: 1}.get(seed, 0)
    finally:
        m.close()


def _box_mesh():
    h = np.array([0.10, 0.075, 0.05])
    v = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * h
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = np.array([t for a, b, c, d in q for t in ((a, b, c), (a, c, d))], np.int32)
    n = v / np.linalg.norm(v, axis=1, keepdims=True)
    return syn.Mesh("box", v.astype(np.float32), n.astype(np.float32), np.zeros((8, 2), np.float32), faces, np.full((2, 2, 3), 100, np.uint8)).finalize()


def test_box_across_many_tiles_and_seams(syn_scene):
    """12 triangles at 0.3 m in 640x480: each covers tens of tiles, every tile seam inside the silhouette is crossed by a triangle"""
    mesh = _box_mesh()
    K = syn.intrinsics()
    pose = syn.pose_matrix(syn.random_rotation(3), (0.02, -0.01, 0.30))
    ref = FR.render(FR.centred(mesh), mesh.faces, pose, K, syn_scene.rgb, syn_scene.depth)
    model = ref["model_mask"] > 0
    H, W = model.shape
    tiles = {(y // TILE, x // TILE) for y, x in zip(*np.nonzero(model))}
    assert len(tiles) >= 20
    tri = ref["tri_id"]
    assert ((tri[:, TILE - 1:W - 1:TILE] == tri[:, TILE:W:TILE]) & (tri[:, TILE:W:TILE] > 0)).any()       # a triangle on both sides of a seam
    assert ((tri[TILE - 1:H - 1:TILE] == tri[TILE:H:TILE]) & (tri[TILE:H:TILE] > 0)).any()
    m = FoundationPose(mesh, K)
    try:
        m.upload_frame(syn_scene.rgb, syn_scene.depth)
        got = _render(m, mesh.name, pose, (H, W))
        border_r = [r for r in range(H) if r % TILE in (0, TILE - 1)]
        border_c = [c for c in range(W) if c % TILE in (0, TILE - 1)]
        _same("box, tile-border rows", {n: a[border_r] for n, a in got.items()}, {n: a[border_r] for n, a in ref.items()})
        _same("box, tile-border columns", {n: a[:, border_c] for n, a in got.items()}, {n: a[:, border_c] for n, a in ref.items()})
        _same("box", got, ref)
        # the same through the Python API (which sizes the outputs by the uploaded frame)
        _same("box, api", m.render_pose(mesh.name, pose), ref)
    finally:
        m.close()


def test_duplicated_and_degenerate_faces():
    base = syn.make_mesh(1)
    W, H = 160, 120
    K = syn.intrinsics(W, H)
    pose = syn.pose_matrix(syn.random_rotation(7), (0.01, 0.0, 0.45))
    rgb = np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)
    depth = np.full((H, W), 1.0, np.float32)
    plain = FR.render(FR.centred(base), base.faces, pose, K, rgb, depth)["tri_id"]
    seen = [int(t) - 1 for t in np.unique(plain) if t > 0]
    a, b = seen[0], seen[-1]
    assert a != b
    # a copy of face a in FRONT of the list (the original, now at a + 1, never wins), a copy of face b at the END (never wins), a face
    # with a repeated index and one with three indices on a line (zero area: two corners equal)
    faces = np.concatenate([base.faces[a:a + 1], base.faces, [[2, 2, 7]], [[5, 9, 5]], base.faces[b:b + 1]]).astype(np.int32)
    mesh = syn.Mesh("dup", base.vertices, base.normals, base.texcoords, faces, base.texture).finalize()
    ref = FR.render(FR.centred(mesh), faces, pose, K, rgb, depth)
    ids = set(int(t) for t in np.unique(ref["tri_id"]))
    assert 1 in ids and (a + 2) not in ids and len(faces) not in ids and (b + 2) in ids
    assert len(faces) - 1 not in ids and len(faces) - 2 not in ids
    assert np.array_equal(ref["model_mask"], np.where(plain > 0, 255, 0))
    m = FoundationPose(mesh, K)
    try:
        m.upload_frame(rgb, depth)
        _same("duplicated + degenerate faces", _render(m, mesh.name, pose, (H, W)), ref)
    finally:
        m.close()


def test_subsets_of_outputs(syn_mesh, syn_scene):
    m = FoundationPose(syn_mesh, syn.intrinsics())
    try:
        m.upload_frame(syn_scene.rgb, syn_scene.depth)
        pose = syn.perturb_pose(syn_scene.gt_pose)
        full = m.render_pose(syn_mesh.name, pose)
        assert set(full) == set(FR.OUTPUTS)
        _same("full call", full, FR.render(FR.centred(syn_mesh), syn_mesh.faces, pose, syn_scene.K, syn_scene.rgb, syn_scene.depth))
        for want in [(n,) for n in FR.OUTPUTS] + [("model_depth", "overlay"), ("visible_mask", "tri_id", "model_mask")]:
            got = _render(m, syn_mesh.name, pose, syn_scene.depth.shape, want=want)
            assert set(got) == set(want)
            _same(f"subset {want}", got, full)
        with pytest.raises(FoundationPoseError, match="no output requested"):
            m.render_pose(syn_mesh.name, pose, want=())
    finally:
        m.close()


def test_device_visible_mask_feeds_a_register(disc_nets, syn_mesh, syn_scene):
    """the re-Register loop of INTEGRATION.md section 5: visible_mask rendered into device memory is the mask of fp_register_ex, nothing
    crosses PCIe; the pose is the one the same mask gives when everything comes from the host"""
    H, W = syn_scene.depth.shape
    m = FoundationPose(syn_mesh, syn.intrinsics(), disc_nets[0], disc_nets[1])
    try:
        rgb_d, depth_d = torch.from_numpy(syn_scene.rgb).cuda(), torch.from_numpy(syn_scene.depth).cuda()
        vis_d = torch.full((H, W), 77, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        m._must(m._L.fp_upload_frame(m._h, C.c_void_p(rgb_d.data_ptr()), C.c_void_p(depth_d.data_ptr()), FP_DEVICE, H, W))
        rec = _lib.FpFrameRender(visible_mask=C.c_void_p(vis_d.data_ptr()))
        p16 = syn.to_colmajor(syn_scene.gt_pose)
        m._must(m._L.fp_render_pose(m._h, syn_mesh.name.encode(), _p(p16), 0.005, C.byref(rec), FP_DEVICE))
        vis = vis_d.cpu().numpy()
        ref = FR.render(FR.centred(syn_mesh), syn_mesh.faces, syn_scene.gt_pose, syn_scene.K, syn_scene.rgb, syn_scene.depth)
        assert np.array_equal(vis, ref["visible_mask"]) and (vis > 0).sum() > 1500
        from_dev = np.zeros(16, np.float32)
        m._must(m._L.fp_register_ex(m._h, C.c_void_p(rgb_d.data_ptr()), C.c_void_p(depth_d.data_ptr()), C.c_void_p(vis_d.data_ptr()), FP_DEVICE,
                                    H, W, syn_mesh.name.encode(), 1, _p(from_dev)))
        ok, from_host = m.Register(syn_scene.rgb, syn_scene.depth, vis, syn_mesh.name)
        assert ok, m.last_error
        assert np.array_equal(syn.from_colmajor(from_dev), from_host)
        torch.cuda.synchronize()
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
    """a Track before and after fp_render_pose on the same model: bit-equal poses, the same launches, the captured graph still there --
    replayed (graphs on) and eager (graphs off)"""
    H, W = syn_scene.depth.shape
    hyp = syn.to_colmajor(syn.perturb_pose(syn_scene.gt_pose))
    m = FoundationPose(syn_mesh, syn.intrinsics(), disc_nets[0], disc_nets[1])
    try:
        rgb_d, depth_d = torch.from_numpy(syn_scene.rgb).cuda(), torch.from_numpy(syn_scene.depth).cuda()
        torch.cuda.synchronize()

        def track():
            out = np.zeros(16, np.float32)
            m._must(m._L.fp_track_ex(m._h, C.c_void_p(rgb_d.data_ptr()), C.c_void_p(depth_d.data_ptr()), FP_DEVICE, H, W, _p(hyp),
                                     syn_mesh.name.encode(), 1, _p(out)))
            return out.tobytes()

        ref = FR.render(FR.centred(syn_mesh), syn_mesh.faces, syn_scene.gt_pose, syn_scene.K, syn_scene.rgb, syn_scene.depth)
        for graphs in (1, 0):
            tl.fpt_model_use_graphs(m._h, graphs)
            first = [track() for _ in range(3)]                  # eager, capturing, replayed
            assert len(set(first)) == 1
            state = tl.fpt_model_graph_state(m._h)
            assert (state & 3) == (3 if graphs else 0)             # bit 0: replay enabled, bit 1: the Track graph exists
            before, log_before = _logged(tl, track)
            # (a device-frame Track leaves the whole frame: the render needs no upload of its own)
            _same(f"render between Tracks, graphs {graphs}", _render(m, syn_mesh.name, syn_scene.gt_pose, (H, W)), ref)
            assert tl.fpt_model_graph_state(m._h) == state, "fp_render_pose dropped a captured graph"
            after, log_after = _logged(tl, track)
            assert before == after == first[0]
            assert log_before == log_after
            assert tl.fpt_model_graph_state(m._h) == state
        m.profile(True)
        _render(m, syn_mesh.name, syn_scene.gt_pose, (H, W))
        rep = m.profile_report()
        m.profile(False)
        assert rep["frame_vertex"]["calls"] == 1 and rep["frame_raster"]["calls"] == 1 and rep["frame_raster"]["bytes"] == H * W * 20.0
    finally:
        m.close()


def test_errors_are_refusals_with_a_message(disc_nets, syn_mesh, syn_scene):
    hw = syn_scene.depth.shape
    pose = syn_scene.gt_pose
    m = FoundationPose(syn_mesh, syn.intrinsics(), disc_nets[0], disc_nets[1])
    try:
        with pytest.raises(FoundationPoseError, match="no frame uploaded"):
            _render(m, syn_mesh.name, pose, hw)
        with pytest.raises(FoundationPoseError, match="no frame uploaded"):
            m.render_pose(syn_mesh.name, pose)
        m.upload_frame(syn_scene.rgb, syn_scene.depth)
        with pytest.raises(FoundationPoseError, match="unknown target_name"):
            _render(m, "nobody", pose, hw)
        for bad in (-0.001, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(FoundationPoseError, match="finite and >= 0"):
                _render(m, syn_mesh.name, pose, hw, tol_m=bad)
        assert _render(m, syn_mesh.name, pose, hw, tol_m=0.0)["model_mask"].any()          # zero is a tolerance
        near = syn.pose_matrix(pose[:3, :3], (0.0, 0.0, 0.05))
        far = syn.pose_matrix(pose[:3, :3], (4000.0, 0.0, 0.2))
        assert FR.refused(FR.centred(syn_mesh), near, syn_scene.K) == "near" and FR.refused(FR.centred(syn_mesh), far, syn_scene.K) == "range"
        for bad, why in ((near, "FP_RENDER_NEAR_M"), (far, "FP_RENDER_SNAP_MAX"), (syn.pose_matrix(pose[:3, :3], (0, 0, -0.7)), "FP_RENDER_NEAR_M")):
            out = np.full(hw, 77, np.uint8)
            rec = _lib.FpFrameRender(model_mask=_p(out))
            with pytest.raises(FoundationPoseError, match=f"pose refused.*{why}"):
                m._must(m._L.fp_render_pose(m._h, syn_mesh.name.encode(), _p(syn.to_colmajor(bad)), 0.005, C.byref(rec), FP_HOST))
            assert (out == 77).all()                                                       # an error, not a picture
        with pytest.raises(FoundationPoseError, match="memspace"):
            rec = _lib.FpFrameRender(model_mask=_p(np.zeros(hw, np.uint8)))
            m._must(m._L.fp_render_pose(m._h, syn_mesh.name.encode(), _p(syn.to_colmajor(pose)), 0.005, C.byref(rec), 2))
        # a Track from a host frame uploads only its crop window: refused like the other stage operators, until the next upload
        ok, _ = m.Track(syn_scene.rgb, syn_scene.depth, syn.perturb_pose(pose), syn_mesh.name)
        assert ok, m.last_error
        with pytest.raises(FoundationPoseError, match="only its crop window"):
            _render(m, syn_mesh.name, pose, hw)
        m.upload_frame(syn_scene.rgb, syn_scene.depth)
        assert _render(m, syn_mesh.name, pose, hw, want=("model_mask",))["model_mask"].any()
    finally:
        m.close()
