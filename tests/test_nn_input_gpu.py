"""The tensor Register and Track actually feed the networks -- nn_in, 2-byte, space-to-depth, [NB2, 84, 84, 32] -- against the CPU oracle.

tests/test_geometry_gpu.py holds the f32 blobs of render_and_transform to the oracle and tests/test_layers_gpu.py takes nn_in as given.
The product never stores those f32 blobs: its rasteriser and crop kernels are other instantiations (80-row strips of 1024 threads from
100 hypotheses, 4-row strips for Track, 8-row strips of 512 / 1024 threads, the fused vertex_crop_kernel up to 4 hypotheses) that pack
six channels to f16 / bf16 and store them through s2d_index.  Here that tensor is taken from the test build's TAP_NN_IN taps (kind 0 = the
refiner's pass, 1 = the scorer's) and every element of it is held to two assertions (tests/nn_in_ref.py), no element exempted:

  oracle   fo.render / fo.crop at the same poses, crop ratio, K and frame: the stored value lies in [rne(ref - 2e-6), rne(ref + 2e-6)]
           (the f32 tensors' own bar, F32_TOL of test_geometry_gpu.py, pushed through the monotone rounding); pad channels and the border are 0
  bits     render_and_transform (the device's f32 path: one template, other store) on the same poses, packed with round-to-nearest-even,
           equals the tensor bit for bit -- this pins strip seams and thread-count variants where the oracle window is a few ulps wide

Poses: Register's refiner pass renders get_hyp_poses(mask)[begin:begin + count] at 1.2 and warps ONE shared crop into the last slot (a
shard of one hypothesis warps its own); its scorer pass renders the refined poses fp_register_shard_begin hands back at 1.1 with a crop
each; Track and track_multi render the pose prior at 1.2.  Graph replay is off: a replayed graph keeps the launches it was captured with."""
import ctypes as C
import gc
from unittest import mock

import numpy as np
import pytest
import torch

import nn_in_ref as R
from geometry_cases import random_case
from foundationpose_cpp_amd import FoundationPose, _lib, synthetic as syn
from foundationpose_cpp_amd.api import FP_DEVICE, FP_HOST, FP_PREC_BF16, FP_PREC_F16, _p
from oracle import fp_oracle as fo

pytestmark = pytest.mark.gpu

TAP_NN_IN = 0       # fp_nn.h enum TapPoint
DEV = "cuda"
PREC = {R.F16: FP_PREC_F16, R.BF16: FP_PREC_BF16}
NAME = {R.F16: "f16", R.BF16: "bf16"}
DTS = [R.F16, R.BF16]


@pytest.fixture(scope="module")
def tl():
    L = _lib.test_lib()
    L.fpt_tap_arm.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    L.fpt_tap_bytes.restype = C.c_longlong
    L.fpt_tap_bytes.argtypes = [C.c_int, C.c_int]
    L.fpt_model_use_graphs.argtypes = [C.c_void_p, C.c_int]
    yield L
    L.fpt_tap_clear()


def _new_model(tl, meshes, K, nets, **kw):
    """a model on the TEST build (its taps act on this instance), graph replay off"""
    with mock.patch.object(_lib, "lib", _lib.test_lib):
        m = FoundationPose(meshes, K, nets[0], nets[1], **kw)
    tl.fpt_model_use_graphs(m._h, 0)
    return m


@pytest.fixture(scope="module")
def model(tl, disc_nets, syn_mesh):
    m = _new_model(tl, syn_mesh, syn.intrinsics(), disc_nets)
    yield m
    m.close()


@pytest.fixture(scope="module")
def om(syn_mesh):
    return fo.OracleMesh(syn_mesh)


@pytest.fixture(scope="module")
def hyp(model, syn_scene):
    model.upload_frame(syn_scene.rgb, syn_scene.depth)
    poses = model.get_hyp_poses(syn_scene.mask)
    assert poses is not None and poses.shape == (252, 4, 4)
    return poses


@pytest.fixture(autouse=True)
def _free_cached_blocks():
    """the model grows its own buffers with hipMalloc: hand the blocks torch's caching allocator keeps back to the runtime"""
    torch.cuda.empty_cache()
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _tapped(tl, dt, call, nb2_refiner=0, nb2_scorer=0):
    """run call() with TAP_NN_IN of the refiner's and / or the scorer's pass armed -> {kind: tensor on the host, element type dt}"""
    tl.fpt_tap_clear()
    bufs = {}
    for kind, nb2 in ((0, nb2_refiner), (1, nb2_scorer)):
        if nb2:
            t = torch.full((nb2, R.P, R.P, 32), float("nan"), dtype=R.TORCH_DT[dt], device=DEV)
            bufs[kind] = t
            assert tl.fpt_tap_arm(kind, TAP_NN_IN, C.c_void_p(t.data_ptr()), t.numel() * t.element_size()) == 0
    torch.cuda.synchronize()
    try:
        call()
        torch.cuda.synchronize()
        for kind, t in bufs.items():
            got = tl.fpt_tap_bytes(kind, TAP_NN_IN)
            assert got == t.numel() * t.element_size(), (kind, got, t.shape)     # the tap was reached, with the size expected
    finally:
        tl.fpt_tap_clear()
    return {kind: t.cpu() for kind, t in bufs.items()}


def _both(case, got, ref, dev, dt):
    """the two assertions on one tensor: ref / dev = (render blobs, crop blobs) of the oracle / of the device's f32 path"""
    ref, dev = np.concatenate(ref), np.concatenate(dev)
    return R.check_oracle(f"{case} vs oracle", got, ref, dt) + R.check_bits(f"{case} vs f32 path", got, dev, dt)


def _report(msgs):
    assert not msgs, "\n".join(msgs)


def _shard_begin(model, scene, name, begin, count):
    """fp_register_shard_begin over hypotheses [begin, begin + count) (refine_itr 1) -> the refined poses it hands back [count, 4, 4]"""
    rgb, depth, mask = model._frame(scene.rgb, scene.depth, scene.mask)
    feat, poses = C.c_void_p(), C.c_void_p()
    model._must(model._L.fp_register_shard_begin(model._h, _p(rgb), _p(depth), _p(mask), FP_HOST, depth.shape[0], depth.shape[1],
                                                 name.encode(), 1, begin, count, C.byref(feat), C.byref(poses)))
    refined = np.zeros((count, 16), np.float32)
    model._must(model._L.fp_download(model._h, _p(refined), poses, refined.nbytes))
    return syn.from_colmajor(refined)


_ORACLE_GRID = {}      # (mesh, float model, grid, K, frame size) -> the oracle's render of the whole hypothesis grid at 1.2


def _register_case(tl, model, mesh, om, scene, hyp, begin, count, dt, subset=None, scorer=True):
    """both passes of Register over hypotheses [begin, begin + count); subset: the hypotheses (indices into the slice) the oracle renders
    -- every element of those images and of the shared crop is checked"""
    case = f"Register {NAME[dt]} [{begin}:{begin + count}]"
    hw = scene.depth.shape
    out = []
    nb2 = count + 1 if count > 1 else 2       # (a shard of one hypothesis warps its own crop)
    T = _tapped(tl, dt, lambda: out.append(_shard_begin(model, scene, mesh.name, begin, count)), nb2, 2 * count if scorer else 0)
    sel = np.arange(count) if subset is None else np.asarray(subset)
    msgs = []
    # refiner pass: the sampler's poses at 1.2, one shared crop in the last slot
    poses = hyp[begin:begin + count][sel]
    p16 = syn.to_colmajor(poses)
    # the sampler gives every hypothesis of the grid the same translation and the observed crop depends on the translation alone: the
    # reference of the shared crop does not depend on which hypothesis the device takes its record from
    assert (hyp[:, :3, 3] == hyp[0, :3, 3]).all(), case
    if subset is None:      # one oracle render of the sampler's grid serves every slice of it, in f16 and bf16
        key = (mesh.name, fo.get_fmad(), hash(hyp.tobytes()), hash(scene.K.tobytes()), hw)
        if key not in _ORACLE_GRID:
            _ORACLE_GRID[key] = fo.render(om, syn.to_colmajor(hyp), scene.K, hw, 1.2)
        ref_a = _ORACLE_GRID[key][begin:begin + count]
    else:
        ref_a = fo.render(om, p16, scene.K, hw, 1.2)
    ref = (ref_a, fo.crop(scene.rgb, scene.depth, scene.K, p16[:1], 1.2, mesh.diameter))
    da, db = model.render_and_transform(mesh.name, poses, 1.2)
    got = torch.cat([T[0][torch.from_numpy(sel)], T[0][count:count + 1]])
    msgs += _both(f"{case} refiner pass", got, ref, (da, db[:1]), dt)
    assert (np.abs(ref[0]).reshape(len(sel), -1).max(1) > 0).all() and np.abs(ref[1]).max() > 0, case      # nothing compared is empty
    if scorer:
        refined = out[0]
        assert np.isfinite(refined).all() and np.abs(refined - hyp[begin:begin + count]).max() > 0, case
        p16 = syn.to_colmajor(refined)
        ref = (fo.render(om, p16, scene.K, hw, 1.1), fo.crop(scene.rgb, scene.depth, scene.K, p16, 1.1, mesh.diameter))
        dev = model.render_and_transform(mesh.name, refined, 1.1)
        msgs += _both(f"{case} scorer pass", T[1], ref, dev, dt)
    return msgs


# ---- Register -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
def test_register_252_both_passes(tl, model, syn_mesh, om, syn_scene, hyp, dt):
    """the headline: 80-row strips of 1024 threads, no row ranges, crop_kernel in the packed mode"""
    model.set_precision(PREC[dt])
    try:
        _report(_register_case(tl, model, syn_mesh, om, syn_scene, hyp, 0, 252, dt))
    finally:
        model.set_precision(FP_PREC_F16)


# every switch of plan_render (fp_geometry.hip), on both sides: 4- vs 8-row strips (2 | 3), the fused
# vertex_crop_kernel vs separate launches (4 | 5), 1024 vs 512 threads (25 | 26), 512 vs 256 threads and 8 vs 20 rows (47 | 48), 20 vs 80 rows
# and with vs without row ranges (99 | 100); slices from the middle of the grid, three of them ending at hypothesis 252
SWITCH_SLICES = [(251, 1), (100, 2), (7, 3), (130, 4), (61, 5), (200, 25), (226, 26), (33, 47), (150, 48), (11, 99), (152, 100)]


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
@pytest.mark.parametrize("begin,count", SWITCH_SLICES)
def test_register_slices_on_both_sides_of_every_launch_switch(tl, model, syn_mesh, om, syn_scene, hyp, begin, count, dt):
    model.set_precision(PREC[dt])
    try:
        _report(_register_case(tl, model, syn_mesh, om, syn_scene, hyp, begin, count, dt))
    finally:
        model.set_precision(FP_PREC_F16)


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
def test_register_1008_refiner_pass(tl, model, syn_mesh, om, syn_scene, dt):
    """inplane steps 24: the oracle renders a seeded subset of 64 hypotheses -- 0, 1007, every multiple of 256 and both its neighbours,
    the rest drawn -- and every element of those images and of the shared crop is held to both assertions"""
    model.set_inplane_steps(24)
    model.set_precision(PREC[dt])
    try:
        assert model.num_hypotheses == 1008
        model.upload_frame(syn_scene.rgb, syn_scene.depth)
        hyp = model.get_hyp_poses(syn_scene.mask)
        fixed = {0, 1007} | {k + d for k in (256, 512, 768) for d in (-1, 0, 1)}
        rest = np.random.default_rng(1008).permutation([i for i in range(1008) if i not in fixed])[:64 - len(fixed)]
        subset = sorted(fixed | {int(i) for i in rest})
        assert len(subset) == 64
        _report(_register_case(tl, model, syn_mesh, om, syn_scene, hyp, 0, 1008, dt, subset=subset, scorer=False))
    finally:
        model.set_precision(FP_PREC_F16)
        model.set_inplane_steps(6)


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
def test_register_5_after_252_holds_nothing_of_the_larger_call(tl, model, syn_mesh, om, syn_scene, hyp, dt):
    model.set_precision(PREC[dt])
    try:
        msgs = _register_case(tl, model, syn_mesh, om, syn_scene, hyp, 0, 252, dt)
        msgs += _register_case(tl, model, syn_mesh, om, syn_scene, hyp, 120, 5, dt)
        _report(msgs)
    finally:
        model.set_precision(FP_PREC_F16)


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
def test_register_20480_triangle_mesh(tl, disc_nets, syn_scene, dt):
    """syn.make_mesh(subdiv=5): the LDS triangle list of a strip fills and is flushed"""
    mesh = syn.make_mesh(subdiv=5, name="fine")
    assert len(mesh.faces) == 20480
    m = _new_model(tl, mesh, syn.intrinsics(), disc_nets)
    try:
        m.set_precision(PREC[dt])
        m.upload_frame(syn_scene.rgb, syn_scene.depth)
        hyp = m.get_hyp_poses(syn_scene.mask)
        om = fo.OracleMesh(mesh)
        msgs = []
        for begin, count in ((0, 252), (192, 60), (100, 12), (7, 1)):
            msgs += _register_case(tl, m, mesh, om, syn_scene, hyp, begin, count, dt)
        _report(msgs)
    finally:
        m.close()


# ---- Track ----------------------------------------------------------------------------------------------------------------------------------

def _track_case(tl, model, mesh, om, K, rgb, depth, pose, dt, case, device_frame=False):
    """one Track (refine_itr 1) at the pose prior: 4-row strips of 1024 threads + vertex_crop_kernel; the frame reaches the crop half as
    the packed window / the rows the host-side estimate chose (device_frame: read whole, in place)"""
    pose = np.asarray(pose, np.float32)
    hw = depth.shape

    def run():
        if device_frame:
            r_d, d_d = torch.from_numpy(rgb).to(DEV), torch.from_numpy(depth).to(DEV)
            out = np.zeros(16, np.float32)
            model._must(model._L.fp_track_ex(model._h, C.c_void_p(r_d.data_ptr()), C.c_void_p(d_d.data_ptr()), FP_DEVICE, hw[0], hw[1],
                                             _p(syn.to_colmajor(pose[None])[0]), mesh.name.encode(), 1, _p(out)))
        else:
            ok, _ = model.Track(rgb, depth, pose, mesh.name)
            assert ok, model.last_error
    T = _tapped(tl, dt, run, 2)
    p16 = syn.to_colmajor(pose[None])
    ref = (fo.render(om, p16, K, hw, 1.2), fo.crop(rgb, depth, K, p16, 1.2, mesh.diameter))
    model.upload_frame(rgb, depth)       # the f32 path reads a whole frame
    dev = model.render_and_transform(mesh.name, pose[None], 1.2)
    return _both(f"Track {NAME[dt]} {case}", T[0], ref, dev, dt)


EDGE_T = [(0.45, 0.3, 0.7), (0.0, 0.0, 0.12), (0.0, 0.0, 0.05), (0.3, -0.2, 5.0), (-0.6, 0.0, 0.7)]   # test_render_edge_cases


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
def test_track_prior_and_edge_poses(tl, model, syn_mesh, om, syn_scene, dt):
    """the perturbed ground truth; partly outside the image, on the near-plane clip path, at 5 m"""
    poses = [("perturbed gt", syn.perturb_pose(syn_scene.gt_pose))]
    Rm = syn.random_rotation(11)
    poses += [(f"edge t={t}", syn.pose_matrix(Rm, t)) for t in EDGE_T]
    model.set_precision(PREC[dt])
    try:
        msgs = []
        for case, p in poses:
            msgs += _track_case(tl, model, syn_mesh, om, syn_scene.K, syn_scene.rgb, syn_scene.depth, p, dt, case)
        _report(msgs)
    finally:
        model.set_precision(FP_PREC_F16)


def test_a_pose_one_millimetre_off_fails_both_assertions_on_both_halves(tl, model, syn_mesh, om, syn_scene):
    """the assertions bite on the device's own content: the tensor of a Track against the references of a pose 1 mm to the side"""
    pose = syn.perturb_pose(syn_scene.gt_pose)
    T = _tapped(tl, R.F16, lambda: model.Track(syn_scene.rgb, syn_scene.depth, pose, syn_mesh.name), 2)
    off = pose.copy()
    off[0, 3] += 0.001
    hw = syn_scene.depth.shape
    model.upload_frame(syn_scene.rgb, syn_scene.depth)
    for p, fails in ((pose, False), (off, True)):
        p16 = syn.to_colmajor(p[None])
        ref = (fo.render(om, p16, syn_scene.K, hw, 1.2), fo.crop(syn_scene.rgb, syn_scene.depth, syn_scene.K, p16, 1.2, syn_mesh.diameter))
        dev = model.render_and_transform(syn_mesh.name, p[None], 1.2)
        for half, name in enumerate(("render", "crop")):
            for msgs in (R.check_oracle(name, T[0][half:half + 1], ref[half], R.F16), R.check_bits(name, T[0][half:half + 1], dev[half], R.F16)):
                assert bool(msgs) == fails, (name, fails, msgs)


# test_track_partial_row_upload_at_the_image_border (tests/test_nn_gpu.py): windows crossing row 0 / row H - 1, outside the frame, 1280x720
BORDER_WINDOWS = [(640, 480, -0.45), (640, 480, 0.45), (640, 480, -0.9), (640, 480, 0.9), (1280, 720, -0.02), (1280, 720, 0.385), (1280, 720, -0.39)]


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
def test_track_windowed_frame_at_the_image_border(tl, disc_nets, syn_mesh, om, dt):
    """a model that has never seen a whole frame: the crop half under FrameRef::pitch / wx0..wy1"""
    msgs = []
    scenes = {(Wd, H): syn.make_scene(syn_mesh, Wd, H) for Wd, H, _ in BORDER_WINDOWS}
    for Wd, H, ty in BORDER_WINDOWS:
        scene = scenes[Wd, H]
        pose = syn.perturb_pose(scene.gt_pose)
        pose[1, 3] = ty
        m = _new_model(tl, syn_mesh, scene.K, disc_nets)
        try:
            m.set_precision(PREC[dt])
            msgs += _track_case(tl, m, syn_mesh, om, scene.K, scene.rgb, scene.depth, pose, dt, f"{Wd}x{H} ty={ty}")
        finally:
            m.close()
    _report(msgs)


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
def test_track_whole_frames_alternate_with_windows(tl, model, syn_mesh, om, dt):
    """one model served from host frames (packed window), device frames (whole, in place) and host frames whose window is too wide to
    be packed (whole rows), on fresh noise: a row or column the window misses would read the frame before, or zero"""
    rng = np.random.default_rng(5)
    K = syn.intrinsics()
    base = syn.perturb_pose(syn.pose_matrix(syn.random_rotation(3), [0, 0, 0.7]).astype(np.float32))
    msgs = []
    model.set_precision(PREC[dt])
    try:
        for k, kind in enumerate(["host", "host", "device", "host", "wide", "host", "device", "wide", "host"]):
            rgb = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
            depth = rng.uniform(0.2, 2.0, (480, 640)).astype(np.float32)
            pose = base.copy()
            tz = 0.25 if kind == "wide" else rng.uniform(0.5, 1.2)
            pose[:3, 3] = [rng.uniform(-0.2, 0.2) * tz, rng.uniform(-0.2, 0.2) * tz, tz]
            msgs += _track_case(tl, model, syn_mesh, om, K, rgb, depth, pose, dt, f"step {k} ({kind})", device_frame=kind == "device")
        _report(msgs)
    finally:
        model.set_precision(FP_PREC_F16)


@pytest.mark.parametrize("seed", range(6))
def test_track_content_nobody_hand_picked(tl, disc_nets, seed):
    """random_case of tests/geometry_cases.py (off-centre mesh, wrap-addressed texture coordinates, fx != fy, noisy depth with holes,
    poses from 0.12 m to 3 m, the six frame sizes), each pose through Track in f16 and bf16"""
    mesh, K, rgb, depth, poses, hw = random_case(seed)
    m = _new_model(tl, mesh, K, disc_nets)
    om = fo.OracleMesh(mesh)
    msgs = []
    try:
        for dt in DTS:
            m.set_precision(PREC[dt])
            for i, p in enumerate(poses):
                msgs += _track_case(tl, m, mesh, om, K, rgb, depth, p, dt, f"random case {seed} pose {i} {hw[1]}x{hw[0]}")
    finally:
        m.close()
    _report(msgs)


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
def test_track_multi_two_meshes(tl, disc_nets, syn_scene, dt):
    """K = 9 and 33 objects of two meshes in alternating groups of three (as test_plan_equals_reality builds them): every object's render
    uses its own mesh, every crop its own record"""
    ma, mb = syn.make_mesh(name="a"), syn.make_mesh(textured=False, name="b", subdiv=3)
    oms = {"a": (ma, fo.OracleMesh(ma)), "b": (mb, fo.OracleMesh(mb))}
    m = _new_model(tl, [ma, mb], syn.intrinsics(), disc_nets)
    hw = syn_scene.depth.shape
    msgs = []
    try:
        m.set_precision(PREC[dt])
        base = syn.perturb_pose(syn_scene.gt_pose)
        for K in (9, 33):
            hyps = np.stack([base] * K)
            hyps[:, 0, 3] += 0.001 * np.arange(K, dtype=np.float32)
            names = [("a", "b")[(k // 3) % 2] for k in range(K)]
            ok = []
            T = _tapped(tl, dt, lambda: ok.append(m.track_multi(syn_scene.rgb, syn_scene.depth, hyps, names)[0]), 2 * K)
            assert ok == [True], m.last_error
            ref_a, ref_b, dev_a, dev_b = ([None] * K for _ in range(4))
            m.upload_frame(syn_scene.rgb, syn_scene.depth)
            for name, (mesh, omesh) in oms.items():
                idx = [k for k in range(K) if names[k] == name]
                p16 = syn.to_colmajor(hyps[idx])
                ra = fo.render(omesh, p16, syn_scene.K, hw, 1.2)
                rb = fo.crop(syn_scene.rgb, syn_scene.depth, syn_scene.K, p16, 1.2, mesh.diameter)
                da, db = m.render_and_transform(name, hyps[idx], 1.2)
                for j, k in enumerate(idx):
                    ref_a[k], ref_b[k], dev_a[k], dev_b[k] = ra[j], rb[j], da[j], db[j]
            msgs += _both(f"track_multi {NAME[dt]} K={K}", T[0], (np.stack(ref_a), np.stack(ref_b)), (np.stack(dev_a), np.stack(dev_b)), dt)
    finally:
        m.close()
    _report(msgs)


# ---- FP_FLOAT_SEPARATE ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
def test_separately_rounded_float_model(tl, model, syn_mesh, om, syn_scene, hyp, dt):
    """set_float_model(0) with fo.set_fmad(False): the FMAD = false instantiations at N = 252 (both passes) and on Track"""
    try:
        model.set_precision(PREC[dt])
        model.set_float_model(0)
        fo.set_fmad(False)
        msgs = _register_case(tl, model, syn_mesh, om, syn_scene, hyp, 0, 252, dt)
        msgs += _track_case(tl, model, syn_mesh, om, syn_scene.K, syn_scene.rgb, syn_scene.depth, syn.perturb_pose(syn_scene.gt_pose), dt,
                            "separately rounded")
        _report(msgs)
    finally:
        fo.set_fmad(True)
        model.set_float_model(1)
        model.set_precision(FP_PREC_F16)
