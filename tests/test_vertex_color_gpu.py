"""Vertex-coloured meshes (fp_set_vertex_colors) on the device: the geometry of a rendering does not change, the
colour follows the host reference tests/vertex_color_ref.py, every production rasteriser schedule packs what the f32 stage form computes,
and Track / track_multi / Register serve a coloured target like a textured one.

Targets of the shared model (test build, graph replay off, the discriminating weights): the session's synthetic mesh `ellipsoid`, its
twin `col` (same geometry and texture, seeded random colour per vertex, colour source VERTEX), `grey` (constant 2x2 texture of value
128: the source of the per-pixel Lambert factor) and `uni` (constant 2x2 texture of the colour UNIFORM)."""
import ctypes as C
import dataclasses
import gc
from unittest import mock

import numpy as np
import pytest
import torch

import nn_in_ref as R
import vertex_color_ref as VR
from foundationpose_cpp_amd import FoundationPose, FoundationPoseError, _lib, synthetic as syn
from foundationpose_cpp_amd.api import FP_COLOR_TEXTURE, FP_COLOR_VERTEX, FP_HOST, FP_PREC_BF16, FP_PREC_F16, _p

pytestmark = pytest.mark.gpu

TAP_NN_IN = 0       # fp_nn.h enum TapPoint
DEV = "cuda"
PREC = {R.F16: FP_PREC_F16, R.BF16: FP_PREC_BF16}
NAME = {R.F16: "f16", R.BF16: "bf16"}
TOL = 2e-6          # the project's bound for shaded channels (VERDICT row a15, F32_TOL of tests/test_geometry_gpu.py)
GREY = 128
UNIFORM = (200, 30, 90)


@pytest.fixture(scope="module")
def tl():
    L = _lib.test_lib()
    L.fpt_tap_arm.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    L.fpt_tap_bytes.restype = C.c_longlong
    L.fpt_tap_bytes.argtypes = [C.c_int, C.c_int]
    L.fpt_model_use_graphs.argtypes = [C.c_void_p, C.c_int]
    yield L
    L.fpt_tap_clear()


@pytest.fixture(scope="module")
def colors(syn_mesh):
    return np.random.default_rng(21).integers(0, 256, (len(syn_mesh.vertices), 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def twin(syn_mesh, colors):
    t = dataclasses.replace(syn_mesh, name="col", vertex_colors=colors)
    t.color_source = FP_COLOR_VERTEX
    return t


def _const_tex(mesh, name, rgb):
    return dataclasses.replace(mesh, name=name, texture=np.broadcast_to(np.uint8(rgb), (2, 2, 3)).copy())


def _test_build_model(tl, meshes, K, nets):
    with mock.patch.object(_lib, "lib", _lib.test_lib):
        m = FoundationPose(meshes, K, *nets)
    tl.fpt_model_use_graphs(m._h, 0)
    return m


@pytest.fixture(scope="module")
def model(tl, disc_nets, syn_mesh, twin, syn_scene):
    meshes = [syn_mesh, twin, _const_tex(syn_mesh, "grey", (GREY,) * 3), _const_tex(syn_mesh, "uni", UNIFORM)]
    m = _test_build_model(tl, meshes, syn.intrinsics(), disc_nets[:2])
    m.upload_frame(syn_scene.rgb, syn_scene.depth)
    yield m
    m.close()


@pytest.fixture(scope="module")
def hyp(model, syn_scene):
    poses = model.get_hyp_poses(syn_scene.mask)
    assert poses is not None and poses.shape == (252, 4, 4)
    return poses


@pytest.fixture(scope="module")
def poses3(syn_scene, hyp):
    return np.stack([syn.perturb_pose(syn_scene.gt_pose), hyp[17], hyp[140]]).astype(np.float32)


@pytest.fixture(autouse=True)
def _free_cached_blocks():
    torch.cuda.empty_cache()
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _tapped(tl, dt, call, nb2):
    """run call() with TAP_NN_IN of the refiner's pass armed -> the tensor [nb2, 84, 84, 32] on the host"""
    tl.fpt_tap_clear()
    t = torch.full((nb2, R.P, R.P, 32), float("nan"), dtype=R.TORCH_DT[dt], device=DEV)
    assert tl.fpt_tap_arm(0, TAP_NN_IN, C.c_void_p(t.data_ptr()), t.numel() * t.element_size()) == 0
    torch.cuda.synchronize()
    try:
        call()
        torch.cuda.synchronize()
        assert tl.fpt_tap_bytes(0, TAP_NN_IN) == t.numel() * t.element_size()      # the tap was reached, with the size expected
    finally:
        tl.fpt_tap_clear()
    return t.cpu()


def _shard_begin(model, scene, name, begin, count):
    rgb, depth, mask = model._frame(scene.rgb, scene.depth, scene.mask)
    feat, poses = C.c_void_p(), C.c_void_p()
    model._must(model._L.fp_register_shard_begin(model._h, _p(rgb), _p(depth), _p(mask), FP_HOST, depth.shape[0], depth.shape[1],
                                                 name.encode(), 1, begin, count, C.byref(feat), C.byref(poses)))


def _pose_err(a, b):
    dR = a[:3, :3] @ b[:3, :3].T
    return np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))), np.linalg.norm(a[:3, 3] - b[:3, 3])


# ---- 1. geometry is untouched ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmad", [1, 0], ids=["fmad", "separate"])
def test_geometry_channels_crop_and_triangle_ids_do_not_change(model, poses3, fmad):
    assert model.color_source("ellipsoid") == FP_COLOR_TEXTURE and model.color_source("col") == FP_COLOR_VERTEX
    model.set_float_model(fmad)
    try:
        for ratio in (1.2, 1.1):
            a_t, b_t = model.render_and_transform("ellipsoid", poses3, ratio)
            a_c, b_c = model.render_and_transform("col", poses3, ratio)
            tri_t, rast_t = model.debug_rasterize("ellipsoid", poses3, ratio)
            tri_c, rast_c = model.debug_rasterize("col", poses3, ratio)
            np.testing.assert_array_equal(b_c.view(np.uint32), b_t.view(np.uint32))
            np.testing.assert_array_equal(a_c[..., 3:].view(np.uint32), a_t[..., 3:].view(np.uint32))
            np.testing.assert_array_equal(tri_c, tri_t)
            np.testing.assert_array_equal(rast_c.view(np.uint32), rast_t.view(np.uint32))
            assert ((tri_t > 0).reshape(3, -1).sum(1) >= 1000).all()
            assert np.abs(a_c[..., :3] - a_t[..., :3]).max() > 0.1            # ... and the colour does
    finally:
        model.set_float_model(1)


# ---- 2. colour against the host reference -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ratio", [1.1, 1.2])
def test_colour_follows_the_host_reference(model, syn_mesh, colors, poses3, ratio):
    got = model.render_and_transform("col", poses3, ratio)[0][..., :3]
    _, rast = model.debug_rasterize("col", poses3, ratio)
    shade = VR.lambert_from_grey(model.render_and_transform("grey", poses3, ratio)[0][..., :3], GREY)
    fg = rast[:, ::-1, :, 3] > 0
    assert (fg.reshape(3, -1).sum(1) >= 1000).all(), fg.reshape(3, -1).sum(1)       # never passes on background
    assert (shade[fg] >= 0.8 - 1e-6).all() and (shade[fg] <= 1.3 + 1e-6).all() and (shade[~fg] == 0).all()

    def err(cols):
        return np.abs(got.astype(np.float64) - VR.render_rgb(rast, syn_mesh.faces, cols, shade)).reshape(3, -1).max(1)
    e = err(colors)
    print(f"crop ratio {ratio}: max |device - reference| per pose {e}")
    assert (e <= TOL).all(), e
    # controls: a reference fed the wrong colours misses the bound on every pose
    assert (err(colors[:, ::-1]) > TOL).all() and (err(np.roll(colors, 1, axis=0)) > TOL).all()


def test_uniform_colour_equals_a_constant_texture(model, colors, poses3):
    uni = np.broadcast_to(np.uint8(UNIFORM), colors.shape).copy()
    model.set_vertex_colors("col", uni)
    try:
        for ratio in (1.1, 1.2):
            a = model.render_and_transform("col", poses3, ratio)[0][..., :3]
            b = model.render_and_transform("uni", poses3, ratio)[0][..., :3]
            assert (b.reshape(3, -1).max(1) > 0.5).all()
            assert np.abs(a.astype(np.float64) - b).max() <= TOL, np.abs(a.astype(np.float64) - b).max()
    finally:
        model.set_vertex_colors("col", colors)


# ---- 3. every production schedule, both element types -----------------------------------------------------------------------------------------

# the smallest N of each rasteriser schedule: 4-row / 1024 threads (Track), 8-row / 1024, 8-row / 512, 20-row / 256, the two 80-row strips
SCHEDULES = [(251, 1), (7, 3), (226, 26), (150, 48), (152, 100)]


@pytest.mark.parametrize("dt", [R.F16, R.BF16], ids=NAME.get)
@pytest.mark.parametrize("begin,count,fmad", [(b, c, 1) for b, c in SCHEDULES] + [(7, 3, 0)])
def test_every_schedule_packs_what_the_f32_stage_form_computes(tl, model, syn_scene, hyp, begin, count, fmad, dt):
    model.set_precision(PREC[dt])
    model.set_float_model(fmad)
    try:
        poses = hyp[begin:begin + count]
        if count == 1:
            poses = syn.perturb_pose(syn_scene.gt_pose)[None]

            def run():
                ok, _ = model.Track(syn_scene.rgb, syn_scene.depth, poses[0], "col")
                assert ok, model.last_error
            T = _tapped(tl, dt, run, 2)
        else:
            T = _tapped(tl, dt, lambda: _shard_begin(model, syn_scene, "col", begin, count), count + 1)
        model.upload_frame(syn_scene.rgb, syn_scene.depth)       # (Track from a host frame uploads its window only)
        dev = model.render_and_transform("col", poses, 1.2)[0]
        tex = model.render_and_transform("ellipsoid", poses, 1.2)[0]
        assert (np.abs(dev[..., :3] - tex[..., :3]).reshape(count, -1).max(1) > 0.1).all()     # it is the coloured rendering that is compared
        msgs = R.check_bits(f"{NAME[dt]} N={count} fmad={fmad}", T[:count], dev, dt)
        assert not msgs, "\n".join(msgs)
        assert R.check_bits("control", T[:count], tex, dt)                                    # the textured rendering would not have passed
    finally:
        model.set_float_model(1)
        model.set_precision(FP_PREC_F16)


# ---- 4. serving paths -----------------------------------------------------------------------------------------------------------------------

def test_track_eager_captured_replayed_and_back_to_the_texture(disc_nets, syn_mesh, twin, colors, syn_scene):
    hypo = syn.perturb_pose(syn_scene.gt_pose)
    plain = FoundationPose(syn_mesh, syn.intrinsics(), *disc_nets[:2])          # never coloured
    served = FoundationPose([syn_mesh, twin], syn.intrinsics(), *disc_nets[:2])

    def track3(m, name):
        out = []
        for _ in range(3):      # eager, capturing, replayed
            ok, p = m.Track(syn_scene.rgb, syn_scene.depth, hypo, name)
            assert ok, m.last_error
            out.append(p)
        assert np.array_equal(out[0], out[1]) and np.array_equal(out[1], out[2])
        return out[0]
    try:
        textured = track3(plain, "ellipsoid")
        coloured = track3(served, "col")
        assert not np.array_equal(coloured, textured)          # the discriminating weights see the colours
        assert np.array_equal(track3(served, "ellipsoid"), textured)
        served.set_vertex_colors("col", None)                  # the twin carries the same texture: now the never-coloured answer
        assert served.color_source("col") == FP_COLOR_TEXTURE
        assert np.array_equal(track3(served, "col"), textured)
        served.set_vertex_colors("col", colors)                # ... and back: the graphs really were dropped
        assert served.color_source("col") == FP_COLOR_VERTEX
        assert np.array_equal(track3(served, "col"), coloured)
    finally:
        plain.close()
        served.close()


def test_track_multi_over_a_textured_and_a_coloured_target(tl, model, syn_scene):
    """one refine-net pass over both crops takes other convolution schedules than N = 1, so the poses agree within the f16 noise bound
    of tests/test_properties_gpu.py; the rendered halves of the networks' input are the single Tracks' bit for bit"""
    base = syn.perturb_pose(syn_scene.gt_pose)
    hyps = np.stack([base, base]).astype(np.float32)
    hyps[1, 0, 3] += 0.002
    names = ["ellipsoid", "col"]
    out = []
    T = _tapped(tl, R.F16, lambda: out.append(model.track_multi(syn_scene.rgb, syn_scene.depth, hyps, names)), 4)
    ok, poses = out[0]
    assert ok, model.last_error
    for k in range(2):
        single = []
        Tk = _tapped(tl, R.F16, lambda: single.append(model.Track(syn_scene.rgb, syn_scene.depth, hyps[k], names[k])), 2)
        assert single[0][0], model.last_error
        assert torch.equal(T[k].view(torch.int16), Tk[0].view(torch.int16)), names[k]
        ang, dist = _pose_err(poses[k], single[0][1])
        assert ang < 0.05 and dist < 5e-5, (names[k], ang, dist)
    model.upload_frame(syn_scene.rgb, syn_scene.depth)


def test_register_42_equals_the_stage_composition_and_sees_the_colours(model, syn_scene):
    model.set_inplane_steps(1)
    try:
        assert model.num_hypotheses == 42
        got = {}
        for name in ("col", "ellipsoid"):
            ok, pose = model.Register(syn_scene.rgb, syn_scene.depth, syn_scene.mask, name)
            assert ok, model.last_error
            got[name] = pose
        # Register spelled with the stage operators (tests/test_properties_gpu.py, _compose_register)
        model.upload_frame(syn_scene.rgb, syn_scene.depth)
        poses = model.get_hyp_poses(syn_scene.mask)
        a, b = model.render_and_transform("col", poses, 1.2)
        t, r = model.refiner_infer(a, b)
        refined = model.refine_post_process("col", poses, t, r)
        a, b = model.render_and_transform("col", refined, 1.1)
        sc = model.scorer_infer(a, b)
    finally:
        model.set_inplane_steps(6)
        model.upload_frame(syn_scene.rgb, syn_scene.depth)
    errs = [_pose_err(got["col"], p) for p in refined]
    idx = int(np.argmin([e[0] + 1e3 * e[1] for e in errs]))
    assert errs[idx][0] < 0.1 and errs[idx][1] < 1e-4, errs[idx]
    assert sc[idx] >= sc.max() - 5e-3, (idx, sc[idx], sc.max())
    assert not np.array_equal(got["col"], got["ellipsoid"])       # the colours reach the networks


# ---- 5. errors ----------------------------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_model_usable_and_geometry_only_models_take_colours(model, twin, colors, poses3, syn_scene):
    expect = model.render_and_transform("col", poses3[:1], 1.2)[0]
    geo = FoundationPose(twin, syn.intrinsics())       # the product build, no networks
    try:
        geo.upload_frame(syn_scene.rgb, syn_scene.depth)
        assert geo.color_source("col") == FP_COLOR_VERTEX
        np.testing.assert_array_equal(geo.render_and_transform("col", poses3[:1], 1.2)[0], expect)
        with pytest.raises(FoundationPoseError, match="unknown target_name"):
            geo.set_vertex_colors("nope", colors)
        with pytest.raises(FoundationPoseError, match="unknown target_name"):
            geo.color_source("nope")
        with pytest.raises(FoundationPoseError, match=rf"got {len(colors) - 1} colours for a target of {len(colors)} vertices"):
            geo.set_vertex_colors("col", colors[:-1])
        with pytest.raises(FoundationPoseError, match=r"\[V,3\]"):
            geo.set_vertex_colors("col", colors.ravel())
        assert geo.color_source("col") == FP_COLOR_VERTEX
        np.testing.assert_array_equal(geo.render_and_transform("col", poses3[:1], 1.2)[0], expect)
        geo.set_vertex_colors("col", None)
        assert geo.color_source("col") == FP_COLOR_TEXTURE
        np.testing.assert_array_equal(geo.render_and_transform("col", poses3[:1], 1.2)[0], model.render_and_transform("ellipsoid", poses3[:1], 1.2)[0])
    finally:
        geo.close()
