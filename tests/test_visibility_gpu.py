"""The device's rasterisers against the float64 ray-cast of tests/visibility_ref.py: the rules R1-R5 of
tests/test_visibility_ref_cpu.py with the outputs of `FoundationPose.debug_rasterize` (the crop rasteriser: raster_shade_kernel /
tri_rows_kernel) and `render_pose` (the frame rasteriser) in the oracle's and the numpy reference's place.

Cases, rules, delta and caps are that module's, imported; nothing is tuned here.  The reference does not depend on the float model: it is
computed once per (case, ratio) and shared.  Every stage-form schedule of plan_render is walked with torus_plate's five poses tiled to
N = 48 (20-row strips with row ranges) and N = 100 (20-row strips without; N = 5 itself is 8-row strips with row ranges), each copy
bit-equal to the N = 5 result, and once more with the row ranges switched off.  The production 2-byte schedules need no run of their
own: tests/test_nn_input_gpu.py holds them bit for bit to this f32 path.  The module prints one table."""
import ctypes as C
from unittest import mock

import numpy as np
import pytest

import test_visibility_ref_cpu as T
import visibility_cases as VC
import visibility_ref as V
from foundationpose_cpp_amd import FoundationPose, _lib

pytestmark = pytest.mark.gpu

_TABLE = []
_STATS = {"crop": ([], []), "frame": ([], [])}          # (the device's statistics, the reference's own on the same images)


@pytest.fixture(scope="module", autouse=True)
def table():
    yield
    print("\n  device against the visibility rules (uncertain = share of (foreground u hit) within delta of an open edge; live = share of the foreground on which R4 can fail):")
    for row in _TABLE:
        T.print_row(*row)
    for kind, (stats, own) in _STATS.items():
        if stats:
            print(f"  {kind}: coverage differs from hit(s) up to D = {max(s['dmax'] for s in stats):.4f} px")
            T.check_aggregate(stats, own, f"device, {kind}")


def _model(c, test_build=False):
    if test_build:
        with mock.patch.object(_lib, "lib", _lib.test_lib):
            m = FoundationPose(c.mesh, c.K)
    else:
        m = FoundationPose(c.mesh, c.K)
    m.upload_frame(c.rgb, c.depth)
    return m


# ---- the crop rasteriser --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VC.GPU_CASES)
def test_crop_rasteriser_obeys_the_visibility_rules(name):
    c = VC.case(name)
    m = _model(c)
    failures = []
    try:
        for fmad in (1, 0):
            m.set_float_model(fmad)
            for ratio in c.ratios:
                refs = T.crop_references(name, ratio)
                own = T.check_images(refs, T.own_images(refs), name)
                try:
                    stats = T.check_images(refs, T.crop_buffers(*m.debug_rasterize(c.mesh.name, c.poses, ratio)), f"{name} ratio {ratio} fmad={fmad}")
                    _TABLE.append(("crop", name, f"ratio {ratio} fmad={fmad}", stats))
                    _STATS["crop"][0].extend(stats)
                    _STATS["crop"][1].extend(own)
                    T.check_caps(stats, name)
                    if name in VC.CLOSED_CASES:
                        assert T.share(stats, "live", "fg") >= T.LIVE_MIN, f"R4 is live on {T.share(stats, 'live', 'fg'):.1%} of the foreground only"
                except AssertionError as e:
                    failures.append(str(e))
    finally:
        m.close()
    assert not failures, "\n".join(failures)


def _tiled(m, c, N, ratio):
    """debug_rasterize of the case's poses tiled to N -> (tri, rast) of the first copy, after asserting every other copy bit-equal to it"""
    P = len(c.poses)
    tri, rast = m.debug_rasterize(c.mesh.name, c.poses[np.arange(N) % P], ratio)
    for n in range(P, N):
        assert np.array_equal(tri[n], tri[n % P]) and np.array_equal(rast[n].view(np.uint32), rast[n % P].view(np.uint32)), f"N = {N}: copy {n} differs from pose {n % P}"
    return tri[:P], rast[:P]


@pytest.mark.parametrize("row_ranges", [1, 0])
def test_every_schedule_of_the_f32_path_gives_the_same_picture(row_ranges):
    """torus_plate's five poses (two across the near plane) at N = 5, 48 and 100: 8-row strips with row ranges, 20-row strips with, 20-row strips
    without -- and all three without row ranges under fpt_set_tri_rows(0).  Every copy equals the N = 5 picture bit for bit, which obeys the rules"""
    c = VC.case("torus_plate")
    L = _lib.test_lib()
    L.fpt_set_tri_rows.argtypes = [C.c_int]
    L.fpt_model_use_graphs.argtypes = [C.c_void_p, C.c_int]
    m = _model(c, test_build=True)
    try:
        L.fpt_model_use_graphs(m._h, 0)              # (a replayed graph would keep the launches it was captured with)
        L.fpt_set_tri_rows(row_ranges)
        for fmad in (1, 0):
            m.set_float_model(fmad)
            for ratio in c.ratios:
                tri5, rast5 = m.debug_rasterize(c.mesh.name, c.poses, ratio)
                stats = T.check_images(T.crop_references(c.name, ratio), T.crop_buffers(tri5, rast5), f"N = 5 rows={row_ranges} ratio {ratio} fmad={fmad}")
                assert sum(s["fg"] for s in stats) > 10000
                for N in (48, 100):
                    tri, rast = _tiled(m, c, N, ratio)
                    assert np.array_equal(tri, tri5) and np.array_equal(rast.view(np.uint32), rast5.view(np.uint32)), f"N = {N} differs from N = 5"
    finally:
        L.fpt_set_tri_rows(1)
        m.close()


# ---- the frame rasteriser ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VC.FRAME_CASES)
def test_frame_rasteriser_obeys_the_visibility_rules(name):
    c = VC.frame_case(name)
    m = FoundationPose(c.mesh, c.K)
    try:
        m.upload_frame(np.zeros(c.hw + (3,), np.uint8), np.zeros(c.hw, np.float32))
        images = []
        for p in c.poses:
            out = m.render_pose(c.mesh.name, p, want=("tri_id", "model_depth"))
            images.append((out["tri_id"].astype(np.int64), out["model_depth"].astype(np.float64)))
    finally:
        m.close()
    refs = T.frame_references(name)
    stats = T.check_images(refs, images, f"frame {name}")
    _TABLE.append(("frame", name, "", stats))
    _STATS["frame"][0].extend(stats)
    _STATS["frame"][1].extend(T.check_images(refs, T.own_images(refs), name))
    T.check_caps(stats, name)


# ---- negative controls on the device's own outputs ----------------------------------------------------------------------------------------------
def test_wrong_rules_fail_on_the_device_outputs_too():
    """the device's pictures of torus_plate against WRONG references -- a near plane at 0.2 m (the device shows what that rule cuts away: R1, R3),
    the farthest surface (R4) -- and with one interior pixel cleared against the right one (R1 + R2)"""
    c = VC.case("torus_plate")
    m = _model(c)
    try:
        images = T.crop_buffers(*m.debug_rasterize(c.mesh.name, c.poses, 1.2))
    finally:
        m.close()
    grids = T.crop_grids(c, 1.2)
    refs = T.crop_references(c.name, 1.2)
    assert not any(s[k] for s in T.check_images(refs, images, "torus_plate") for k in V.RULES)
    for n in VC.NEAR_POSES[c.name]:
        s = V.check(V.reference(c.mesh, c.poses[n], c.K, grids[n], V.DELTA_CROP, znear=0.2), *images[n])
        assert s["R1"] > 0 and s["R3"] > 0, s
    for n in range(len(c.poses)):
        tid, zw = images[n]
        s = V.check(V.reference(c.mesh, c.poses[n], c.K, grids[n], V.DELTA_CROP, sense=-1.0), tid, -zw)
        assert s["R4"] > 0 and s["R1"] == s["R2"] == s["R3"] == 0, s
        inner = np.argwhere((refs[n].n_certain > 0) & (refs[n].D > refs[n].delta) & (tid > 0))
        t = tid.copy()
        t[tuple(inner[len(inner) // 2])] = 0
        s = V.check(refs[n], t, zw)
        assert (s["R1"], s["R2"], s["R3"], s["R4"]) == (1, 1, 0, 0), s
