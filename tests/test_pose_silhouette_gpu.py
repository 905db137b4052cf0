"""fp_mask_distance and fp_pose_silhouette against tests/silhouette_ref.py: EQUAL in every integer, in the status
and in the bits of the three floats -- the device produces integers only and the host rounds once, so there is no tolerance to choose.
The cases are those of tests/silhouette_cases.py, which tests/test_silhouette_ref_cpu.py holds to a second distance transform and to hand
answers.  Then the promises of the interface: byte-identical records whatever the batch or the chunking, refusals per record and per
call, the untouched serving path, and neighbours on one model that leave nothing behind."""
import ctypes as C
import os
import re
from unittest import mock

import numpy as np
import pytest

import icp_cases as IC
import silhouette_cases as SIC
import silhouette_ref as SR
import test_stage_scratch_gpu as SS
from foundationpose_cpp_amd import FoundationPose, FoundationPoseError, PoseSilhouette, _lib, synthetic as syn
from foundationpose_cpp_amd.api import _p

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "foundationpose_amd.h")).read()
FP_HOST, FP_DEVICE = 0, 1


def _const(name):
    return int(re.search(rf"#define {name} (\d+)", HEADER).group(1))


def _raw(m, name, mask, poses, tol=SIC.TOL, trunc=0, flags=0, N=None, out=None, memspace=FP_HOST):
    """fp_pose_silhouette through the raw ABI -> (return code, records).  mask: a u8 array, or a device address with memspace=FP_DEVICE"""
    e = syn.to_colmajor(np.asarray(poses, np.float32).reshape(-1, 4, 4))
    N = len(e) if N is None else N
    out = (_lib.FpPoseSilhouette * max(N, 1))() if out is None else out
    if isinstance(mask, np.ndarray):
        mask = np.ascontiguousarray(mask, np.uint8)
        ptr = _p(mask)
    else:
        ptr = mask
    return m._L.fp_pose_silhouette(m._h, None if name is None else name.encode(), ptr, memspace, _p(e), N, tol, trunc, flags, out), out


def _sil(m, name, mask, poses, **kw):
    rc, out = _raw(m, name, mask, poses, **kw)
    m._must(rc)
    return list(out)


def _bytes(rec):
    return b"".join(bytes(r) for r in rec) if isinstance(rec, (list, tuple)) else bytes(rec)


def _equal(what, got, ref):
    """one device record against the reference's dict: every integer, the status, and the bits of the three floats"""
    print(f"{what}: device " + " ".join(f"{k}={getattr(got, k)}" for k in SR.INTS) + f" iou={float(got.iou):.6f}")
    for k in SR.INTS:
        assert getattr(got, k) == ref[k], (what, k, getattr(got, k), ref[k])
    for k in SR.FLOATS:
        assert np.float32(getattr(got, k)).tobytes() == np.float32(ref[k]).tobytes(), (what, k, getattr(got, k), ref[k])
    assert got.reserved == 0 and got.reserved_f == 0.0


def _run_case(m, name, **kw):
    c = SIC.case(name)
    m.upload_frame(np.zeros(c["D"].shape + (3,), np.uint8), c["D"])
    return _sil(m, c["mesh"].name, c["mask"], c["poses"], tol=c["tol"], trunc=c["trunc"], flags=1 if c["amodal"] else 0, **kw)


@pytest.fixture(scope="module")
def model():
    m = FoundationPose([IC.ico(1), IC.ico(2), IC.ico(3), SIC.hand_quad()], SIC.K)          # geometry-only
    yield m
    m.close()


# ---- the distance transform alone -----------------------------------------------------------------------------------------------------
def _distance(m, mask, want=(True, True)):
    mask = np.ascontiguousarray(mask, np.uint8)
    a, b = (np.full(mask.shape, 0x5A5A5A5A, np.uint32) if w else None for w in want)
    m._must(m._L.fp_mask_distance(m._h, _p(mask), FP_HOST, _p(a), _p(b)))
    return a, b


@pytest.mark.parametrize("name", SIC.GPU_MASKS)
def test_mask_distance_equals_brute_force(model, name):
    mask = SIC.mask_case(name)
    model.upload_frame(np.zeros(mask.shape + (3,), np.uint8), np.zeros(mask.shape, np.float32))
    keep = mask.copy()
    a, b = _distance(model, mask)
    ra, rb = SIC.mask_expected(name)
    print(f"{name}: {mask.shape}, {int((mask > 0).sum())} mask pixels, largest d2 {int(ra.max())} / {int(rb.max())}")
    assert np.array_equal(a.astype(np.int64), ra) and np.array_equal(b.astype(np.int64), rb)
    assert np.array_equal(mask, keep)
    # each output alone, and through the Python interface
    only_a, none_b = _distance(model, mask, (True, False))
    none_a, only_b = _distance(model, mask, (False, True))
    assert none_a is None and none_b is None and np.array_equal(only_a, a) and np.array_equal(only_b, b)
    pa, pb = model.mask_distance(mask)
    assert pa.dtype == np.uint32 and np.array_equal(pa, a) and np.array_equal(pb, b)


def _device_copy(host):
    """a torch tensor on the GPU holding `host` (the library reads its address)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(host)).cuda()


@pytest.mark.parametrize("name", ("scene_mask", "3x1300"))
def test_a_device_mask_gives_the_same(model, name):
    mask = SIC.mask_case(name)
    model.upload_frame(np.zeros(mask.shape + (3,), np.uint8), np.zeros(mask.shape, np.float32))
    dev = _device_copy(mask)
    import torch
    torch.cuda.synchronize()
    a, b = (np.zeros(mask.shape, np.uint32) for _ in range(2))
    model._must(model._L.fp_mask_distance(model._h, C.c_void_p(dev.data_ptr()), FP_DEVICE, _p(a), _p(b)))
    ra, rb = SIC.mask_expected(name)
    assert np.array_equal(a.astype(np.int64), ra) and np.array_equal(b.astype(np.int64), rb)
    assert np.array_equal(dev.cpu().numpy(), mask)                                    # the caller's mask is not modified
    if name == "scene_mask":
        c = SIC.case("scene_1")
        model.upload_frame(np.zeros(c["D"].shape + (3,), np.uint8), c["D"])
        host = _sil(model, c["mesh"].name, c["mask"], c["poses"])
        there = _sil(model, c["mesh"].name, C.c_void_p(dev.data_ptr()), c["poses"], memspace=FP_DEVICE)
        assert _bytes(host) == _bytes(there)
        assert np.array_equal(dev.cpu().numpy(), mask)


def test_mask_distance_refusals(model):
    mask = SIC.mask_case("random_half")
    a = np.full(mask.shape, 0x5A5A5A5A, np.uint32)
    fresh = FoundationPose(IC.ico(1), SIC.K, max_input_image_width=8200)
    skew = np.array(SIC.K, np.float32)
    skew[0, 1] = 0.5
    ms = FoundationPose(IC.ico(1), skew)
    try:
        def refused(match, m, *args):
            rc = m._L.fp_mask_distance(m._h, *args)
            assert rc != 0 and re.search(match, _lib.last_error()), (match, rc, _lib.last_error())
            assert (a == 0x5A5A5A5A).all()

        refused("no frame uploaded", fresh, _p(mask), FP_HOST, _p(a), None)
        fresh.upload_frame(np.zeros(mask.shape + (3,), np.uint8), np.zeros(mask.shape, np.float32))
        ms.upload_frame(np.zeros(mask.shape + (3,), np.uint8), np.zeros(mask.shape, np.float32))
        refused("invalid arguments", fresh, None, FP_HOST, _p(a), None)
        refused("invalid arguments", fresh, _p(mask), FP_HOST, None, None)
        refused("memspace", fresh, _p(mask), 2, _p(a), None)
        refused(r"fp_mask_distance: the model's K is not a plain pinhole matrix: K\[1\]", ms, _p(mask), FP_HOST, _p(a), None)
        wide = np.zeros((1, 8193), np.uint8)
        fresh.upload_frame(np.zeros((1, 8193, 3), np.uint8), np.zeros((1, 8193), np.float32))
        refused("FP_SIL_MAX_DIM", fresh, _p(wide), FP_HOST, _p(a), None)
        out = (_lib.FpPoseSilhouette * 1)()
        C.memset(out, 0x5A, C.sizeof(out))
        rc, _ = _raw(fresh, IC.ico(1).name, wide, [IC.ICO_G], out=out)
        assert rc != 0 and "FP_SIL_MAX_DIM" in _lib.last_error() and _bytes(out) == b"\x5a" * 64
        with pytest.raises(FoundationPoseError, match="a mask of shape"):
            fresh.mask_distance(mask)
    finally:
        fresh.close()
        ms.close()


# ---- the records ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in SIC.CASES if n != "batch_512"])
def test_cases_equal_the_reference(model, name):
    got, ref = _run_case(model, name), SIC.expected(name)
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        _equal(f"{name}[{i}]", g, r)
    if name.startswith("scene_"):
        assert got[0].iou >= 0.98 and all(g.iou < got[0].iou for g in got[1:])
    if name.startswith("hand_quad"):
        _equal(name, got[0], SIC.hand_quad_expected(SIC.case(name)["trunc"]))


def test_what_the_cases_cover():
    """the cases do reach the paths they are named for (checked on the reference: nothing here needs the device twice)"""
    ex = SIC.expected
    assert [r["status"] for r in ex("refused")] == [0, 1, 0, 2, 0]
    for r in (ex("refused")[1], ex("refused")[3]):
        assert all(r[k] == 0 for k in SR.INTS if k != "status") and r["iou"] == 0
    out = ex("outside")[0]                                                            # wholly outside: only the mask's own numbers
    assert out["status"] == 0 and out["n_model"] == out["n_visible"] == out["n_inter"] == out["n_spill"] == 0 and out["n_mask"] == out["n_miss"] > 500
    assert out["sum_spill_d2"] == 0 and out["sum_miss_d2"] > 0 and out["iou"] == 0 and out["rms_miss_px"] > 0
    e = ex("outside_empty_mask")
    assert e[0]["status"] == SR.EMPTY and e[1]["status"] == 0 and e[1]["n_spill"] == e[1]["n_visible"] > 500
    assert e[1]["sum_spill_d2"] == e[1]["n_spill"] * SR.D2_NONE > 2 ** 32                 # no mask pixel anywhere: every spill pixel is D2_NONE away
    f = ex("full_mask")[0]
    assert f["n_spill"] == 0 and f["n_mask"] == SIC.W * SIC.H and f["sum_miss_d2"] == f["n_miss"] * SR.D2_NONE
    assert ex("full_mask_trunc")[0]["sum_miss_d2"] == ex("full_mask_trunc")[0]["n_miss"] * 9
    assert ex("wall")[0]["n_visible"] < ex("wall_amodal")[0]["n_visible"] == ex("wall_amodal")[0]["n_model"]
    assert ex("nan_zero_inf")[0]["n_visible"] == ex("nan_zero_inf")[0]["n_model"] > 500
    edge, gone = ex("ragged")[3], ex("ragged")[5]
    assert 0 < edge["n_model"] < ex("ragged")[0]["n_model"] and gone["n_model"] == 0


@pytest.fixture
def tl():
    """the test build (its chunk hooks and launch log) as THE library of the models made inside the test"""
    L = _lib.test_lib()
    for hook in ("fpt_silhouette_set_chunk", "fpt_color_set_chunk", "fpt_vsd_set_chunk", "fpt_icp_set_chunk"):
        getattr(L, hook).argtypes = [C.c_int]
        getattr(L, hook).restype = None
    L.fpt_launch_log_arm.argtypes = [C.c_int]
    L.fpt_launch_log_get_all.argtypes = [C.POINTER(C.c_int), C.c_char_p, C.c_int, C.c_int]
    with mock.patch.object(_lib, "lib", _lib.test_lib):
        yield L
    L.fpt_silhouette_set_chunk(0)


@pytest.mark.parametrize("name,chunks", (("batch_47", (1, 5, 46)), ("batch_512", (100, 511))))
def test_batches_across_chunk_boundaries(tl, name, chunks):
    """47 and 512 poses, whole and in forced chunks that do not divide them: every record equals the reference, whatever the seams"""
    c = SIC.case(name)
    m = FoundationPose(c["mesh"], SIC.K)
    try:
        m.upload_frame(np.zeros(c["D"].shape + (3,), np.uint8), c["D"])
        whole = _sil(m, c["mesh"].name, c["mask"], c["poses"])
        ref = SIC.expected(name)
        assert len(whole) == len(ref) == int(name[6:])
        for i, (g, r) in enumerate(zip(whole, ref)):
            for k in SR.INTS:
                assert getattr(g, k) == r[k], (name, i, k, getattr(g, k), r[k])
            for k in SR.FLOATS:
                assert np.float32(getattr(g, k)).tobytes() == np.float32(r[k]).tobytes(), (name, i, k)
        assert len({_bytes(r) for r in whole}) > len(whole) // 2                     # (the poses do differ)
        for chunk in chunks:
            tl.fpt_silhouette_set_chunk(chunk)
            assert _bytes(_sil(m, c["mesh"].name, c["mask"], c["poses"])) == _bytes(whole), chunk
        tl.fpt_silhouette_set_chunk(0)
    finally:
        m.close()


def test_a_record_is_the_same_alone_in_any_batch_and_again(model):
    c = SIC.case("ragged")
    name, poses, mask = c["mesh"].name, c["poses"], c["mask"]
    model.upload_frame(np.zeros(c["D"].shape + (3,), np.uint8), c["D"])
    batch = _sil(model, name, mask, poses, trunc=3)
    assert len({_bytes(r) for r in batch}) == 7
    assert _bytes(batch) == _bytes(_sil(model, name, mask, poses, trunc=3))          # call to call
    three = _sil(model, name, mask, poses[[0, 3, 6]], trunc=3)
    for k, i in enumerate((0, 3, 6)):
        alone = _sil(model, name, mask, poses[i:i + 1], trunc=3)
        assert _bytes(alone[0]) == _bytes(batch[i]) == _bytes(three[k]), i


def test_refused_poses_do_not_disturb_their_neighbours(model):
    c = SIC.case("refused")
    got = _run_case(model, "refused")
    assert [g.status for g in got] == [0, 1, 0, 2, 0]
    for g in (got[1], got[3]):
        assert bytes(g)[:24] == b"\0" * 24 and bytes(g)[28:] == b"\0" * 36
    clean = _sil(model, c["mesh"].name, c["mask"], c["poses"][[0, 2, 4]])
    assert _bytes([got[0], got[2], got[4]]) == _bytes(clean)


def test_the_depth_filter_does_not_reach_the_call():
    c = SIC.case("nan_zero_inf")
    m = FoundationPose(c["mesh"], SIC.K)
    try:
        rgb = np.zeros(c["D"].shape + (3,), np.uint8)
        m.upload_frame(rgb, c["D"])
        off = _sil(m, c["mesh"].name, c["mask"], c["poses"])
        m.set_depth_filter(True)
        on = _sil(m, c["mesh"].name, c["mask"], c["poses"])
        m.upload_frame(rgb, c["D"])
        again = _sil(m, c["mesh"].name, c["mask"], c["poses"])
        assert _bytes(off) == _bytes(on) == _bytes(again)
        _equal("depth filter on", on[0], SIC.expected("nan_zero_inf")[0])
    finally:
        m.close()


def test_refusals_leave_out_untouched():
    c = SIC.case("ragged")
    G, mask = c["poses"][0], c["mask"]
    max_batch, cap = _const("FP_MAX_BATCH"), int(re.search(r"#define FP_SIL_MAX_WORK (\d+)LL", HEADER).group(1))
    # the work cap: every pose so near that its bound is the whole 1920 x 1080 frame (2040 tiles), a mesh of F degenerate faces
    tiles = 60 * 34
    F = cap // (max_batch * tiles) + 1
    base = c["mesh"]
    many = syn.Mesh("many", base.vertices, base.normals, base.texcoords, np.zeros((F, 3), np.int32), base.texture).finalize()
    near = IC.pose(np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]]), (0.0, 0.0, 0.09))   # the bounding sphere reaches the camera plane, no vertex does
    m = FoundationPose([base, many], SIC.K)
    skew = np.array(SIC.K, np.float32)
    skew[0, 1] = 0.5
    ms = FoundationPose(base, skew)
    try:
        def refused(match, *a, model=m, **kw):
            n = max(kw.get("N") or 1, len(np.asarray(a[2]).reshape(-1, 4, 4)))
            out = (_lib.FpPoseSilhouette * n)()
            C.memset(out, 0x5A, C.sizeof(out))
            before = _bytes(out)
            rc, _ = _raw(model, *a, out=out, **kw)
            assert rc != 0 and re.search(match, _lib.last_error()), (match, rc, _lib.last_error())
            assert _bytes(out) == before

        refused("fp_pose_silhouette: no frame uploaded", base.name, mask, [G])
        rgb = np.zeros(c["D"].shape + (3,), np.uint8)
        m.upload_frame(rgb, c["D"])
        ms.upload_frame(rgb, c["D"])
        assert _raw(m, base.name, mask, [G])[0] == 0
        refused(r"fp_pose_silhouette: the model's K is not a plain pinhole matrix: K\[1\]", base.name, mask, [G], model=ms)
        refused("unknown target_name", "nobody", mask, [G])
        refused("fp_pose_silhouette: invalid arguments", base.name, None, [G])
        refused("fp_pose_silhouette: memspace", base.name, mask, [G], memspace=7)
        refused(r"fp_pose_silhouette: 0 poses \(1\.\.FP_MAX_BATCH", base.name, mask, [G], N=0)
        refused(r"1\.\.FP_MAX_BATCH", base.name, mask, [G] * (max_batch + 1))
        for value in (float("nan"), float("inf"), -0.01):
            refused("fp_pose_silhouette: tol_m", base.name, mask, [G], tol=value)
            refused("fp_pose_silhouette: tol_m", base.name, mask, [G], tol=value, flags=1)   # checked even where it is not used
        assert _raw(m, base.name, mask, [G], tol=0.0)[0] == 0
        for value in (-1, 32768):
            refused("fp_pose_silhouette: trunc_px", base.name, mask, [G], trunc=value)
        assert _raw(m, base.name, mask, [G], trunc=32767)[0] == 0
        for value in (2, 3, -1, 1 << 20):
            refused("fp_pose_silhouette: unknown flag bits", base.name, mask, [G], flags=value)
        for value in (float("nan"), float("inf"), -float("inf")):
            for where in ((0, 0), (2, 3), (3, 3)):
                bad = np.array(G)
                bad[where] = value
                refused(r"fp_pose_silhouette: a non-finite entry in poses\[1\]", base.name, mask, [G, bad])
        # the cap: FP_MAX_BATCH poses over the whole of a large frame are one face too many; nothing is launched
        big = np.zeros((1080, 1920), np.uint8)
        m.upload_frame(np.zeros((1080, 1920, 3), np.uint8), np.zeros((1080, 1920), np.float32))
        assert max_batch * tiles * F > cap >= max_batch * tiles * (F - 1)
        refused("FP_SIL_MAX_WORK", "many", big, [near] * max_batch)
        rc, out = _raw(m, "many", big, [near])
        assert rc == 0 and out[0].n_model == 0 and out[0].status == SR.EMPTY
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
    frame leaves only its crop window, and a submitted Track is pending: both refuse fp_pose_silhouette"""
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
        out = (_lib.FpPoseSilhouette * 1)()
        C.memset(out, 0x5A, C.sizeof(out))
        rc, _ = _raw(m, syn_mesh.name, syn_scene.mask, [pose], out=out)
        assert rc != 0 and "only its crop window" in _lib.last_error() and _bytes(out) == b"\x5a" * C.sizeof(out)
        m.upload_frame(syn_scene.rgb, syn_scene.depth)
        G = syn_scene.gt_pose
        m.profile_reset(); m.profile(True)
        recs = m.pose_silhouette(syn_mesh.name, syn_scene.mask, [pose, G], trunc_px=8)
        rep = m.profile_report()
        m.profile(False)
        for fam in ("mask_edt_cols", "mask_edt_rows", "silhouette_vertex", "silhouette_tile"):
            assert rep[fam]["calls"] == 1, fam
        d2m, d2b = m.mask_distance(syn_scene.mask)
        assert isinstance(recs[1], PoseSilhouette) and recs[1].status == 0 and recs[1].n_mask == int((syn_scene.mask > 0).sum())
        assert recs[1].iou > 0.95 and recs[1].n_visible == recs[1].n_inter + recs[1].n_spill and recs[1].n_miss == recs[1].n_mask - recs[1].n_inter
        on = syn_scene.mask > 0
        assert np.array_equal(d2m == 0, on) and np.array_equal(d2b == 0, ~on)
        print(f"640 x 480 scene: iou of the truth {recs[1].iou:.4f} (spill {recs[1].n_spill}, miss {recs[1].n_miss}), of the tracked pose {recs[0].iou:.4f}")
        after, log_after = _logged(tl, serve)
        assert after[0] == before[0][0] and log_after == log_before
        hyp = syn.to_colmajor(syn.perturb_pose(syn_scene.gt_pose))
        m._must(m._L.fp_track_submit(m._h, _p(syn_scene.rgb), _p(syn_scene.depth), 0, hw[0], hw[1], _p(hyp), syn_mesh.name.encode(), 1))
        rc, _ = _raw(m, syn_mesh.name, syn_scene.mask, [pose], out=out)
        assert rc != 0 and "has not been waited for" in _lib.last_error() and _bytes(out) == b"\x5a" * C.sizeof(out)
        m._must(m._L.fp_track_wait(m._h, _p(np.zeros(16, np.float32))))
    finally:
        m.close()


def _color(m, name, poses):
    e = syn.to_colmajor(np.asarray(poses, np.float32).reshape(-1, 4, 4))
    out = (_lib.FpPoseColor * len(e))()
    m._must(m._L.fp_pose_color(m._h, name.encode(), _p(e), len(e), SIC.TOL, out))
    return bytes(out)


def test_neighbours_on_one_model_leave_nothing_behind(tl):
    """in the spirit of tests/test_stage_scratch_gpu.py (its window, its poses): fp_pose_color, fp_pose_silhouette, fp_refine_depth,
    fp_mask_distance and the first two again on ONE model each equal the same call on a fresh model"""
    small, large = syn.make_mesh(1, textured=True, name="ico1t"), syn.make_mesh(3, textured=True, name="ico3t")
    mask = np.zeros((SS.H, SS.W), np.uint8)
    mask[20:60, 30:75] = 255

    def fresh():
        m = FoundationPose([small, large], SS.K)
        m.upload_frame(SS.RGB, SS.DEPTH)
        return m

    steps = [("pose_color, large mesh, chunks of 2", {"fpt_color_set_chunk": 2}, lambda m: _color(m, large.name, SS.EST)),
             ("pose_silhouette, large mesh, chunks of 2", {"fpt_silhouette_set_chunk": 2}, lambda m: _bytes(_sil(m, large.name, mask, SS.EST))),
             ("refine_depth, small mesh, chunks of 2", {"fpt_icp_set_chunk": 2}, lambda m: SS._refine(m, small.name, SS.EST, 2)),
             ("mask_distance", {}, lambda m: b"".join(a.tobytes() for a in m.mask_distance(mask))),
             ("pose_silhouette, small mesh, amodal", {}, lambda m: _bytes(_sil(m, small.name, mask, SS.EST[:2], trunc=2, flags=1))),
             ("pose_color, small mesh", {}, lambda m: _color(m, small.name, SS.EST[:2])),
             ("refine_depth, large mesh", {}, lambda m: SS._refine(m, large.name, SS.EST[:2], 2))]
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
    first = _lib.FpPoseSilhouette.from_buffer_copy(got[1][:64])
    _equal("pose_silhouette on the shared model", first, SR.records(large, SS.EST[:1], SS.K, SS.DEPTH, mask, SIC.TOL)[0])


def test_through_the_python_interface(model):
    c = SIC.case("ragged")
    model.upload_frame(np.zeros(c["D"].shape + (3,), np.uint8), c["D"])
    recs = model.pose_silhouette(c["mesh"].name, c["mask"], c["poses"], trunc_px=3, amodal=True)
    raw = _sil(model, c["mesh"].name, c["mask"], c["poses"], trunc=3, flags=1)
    assert len(recs) == 7 and all(isinstance(r, PoseSilhouette) for r in recs)
    for r, w in zip(recs, raw):
        assert [getattr(r, k) for k in SR.INTS] == [getattr(w, k) for k in SR.INTS]
        assert all(np.float32(getattr(r, k)) == np.float32(getattr(w, k)) for k in SR.FLOATS)
    with pytest.raises(FoundationPoseError, match="unknown target_name"):
        model.pose_silhouette("nobody", c["mask"], c["poses"])
    with pytest.raises(FoundationPoseError, match="a mask of shape"):
        model.pose_silhouette(c["mesh"].name, c["mask"][:10], c["poses"])
