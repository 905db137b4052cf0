"""The depth filter option (fp_set_depth_filter) without a GPU.

  symbols   header, library, Python class and both C++ wrappers carry the setter and the getter
  window    plan_track_window (asked through the test build's fpt_plan_track_window): reach 0 reproduces the estimate Track made before
            the function existed (tests/depth_filter_cases.py window_before), reach 4 grows every side by 4 and clamps, and which outcome
            it is -- whole frame, outside the frame, rows, rectangle -- never depends on the reach
  inputs    the synthetic scenes the GPU tests run the option on keep most of the object after the filter, and the filter changes it:
            a condition on the tests' inputs (with the oracle alone), not a bar on the device"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import depth_filter_cases as DC
from foundationpose_cpp_amd import FoundationPose, _lib, synthetic as syn
from oracle import fp_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_T = [(0.45, 0.3, 0.7), (0.0, 0.0, 0.12), (0.0, 0.0, 0.05), (0.3, -0.2, 5.0), (-0.6, 0.0, 0.7)]      # tests/test_nn_input_gpu.py
BORDER_WINDOWS = [(640, 480, -0.45), (640, 480, 0.45), (640, 480, -0.9), (640, 480, 0.9), (1280, 720, -0.02), (1280, 720, 0.385), (1280, 720, -0.39)]
SIZES = [(640, 480), (1280, 720)]


@pytest.fixture(scope="module")
def scenes(syn_mesh):
    return {wh: syn.make_scene(syn_mesh, *wh) for wh in SIZES}


# ---- symbols ----------------------------------------------------------------------------------------------------------------------------

def test_header_library_and_python_carry_the_option():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "foundationpose_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+fp_set_depth_filter\s*\(\s*fp_model\s*\*\s*m\s*,\s*int\s+on\s*\)\s*;", header)
    assert re.search(r"\bint\s+fp_get_depth_filter\s*\(\s*const\s+fp_model\s*\*\s*m\s*\)\s*;", header)
    for L in (_lib.lib(), _lib.test_lib()):
        assert hasattr(L, "fp_set_depth_filter") and hasattr(L, "fp_get_depth_filter")
    assert callable(FoundationPose.set_depth_filter) and callable(FoundationPose.depth_filter)
    # refusals that need no device: a null model
    L = _lib.lib()
    assert L.fp_set_depth_filter(None, 1) != 0 and b"null model" in L.fp_last_error()
    assert L.fp_get_depth_filter(None) < 0


WRAPPER_SRC = r'''
#include <cstdio>
#include "foundationpose_amd.hpp"
int main() {
  fp_amd::Mesh m;
  m.name = "tri";
  m.vertices = {0,0,0, 0.1f,0,0, 0,0.1f,0};
  m.normals = {0,0,-1, 0,0,-1, 0,0,-1};
  m.texcoords = {0,0, 1,0, 0,1};
  m.faces = {0,1,2};
  m.texture = std::vector<uint8_t>(12, 100);
  m.tex_height = 2; m.tex_width = 2; m.diameter = 0.1414f;
  const float K[9] = {320,0,320, 0,320,240, 0,0,1};
  try {
    fp_amd::FoundationPose fp({m}, K, "", "");
    const bool off0 = !fp.DepthFilter(), on = fp.SetDepthFilter(true) && fp.DepthFilter(), off1 = fp.SetDepthFilter(false) && !fp.DepthFilter();
    std::printf("depth filter: off by default=%d on=%d off again=%d\n", (int)off0, (int)on, (int)off1);
    return off0 && on && off1 ? 0 : 4;
  } catch (const std::runtime_error &e) {
    std::printf("threw: %s\n", e.what());
    return 0;
  }
}
'''
SHIM_SRC = r'''
#include "detection_6d_foundationpose_amd.hpp"
bool toggle(detection_6d::FoundationPoseAmd &m) { return m.SetDepthFilter(true) && m.DepthFilter() && m.SetDepthFilter(false) && !m.DepthFilter(); }
int main() { return 0; }
'''


def test_cpp_wrappers_compile_with_a_call(tmp_path):
    libdir = os.path.join(ROOT, "foundationpose_cpp_amd")
    link = ["-L", libdir, "-lfoundationpose_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    (tmp_path / "w.cpp").write_text(WRAPPER_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(tmp_path / "w.cpp"), "-o", str(tmp_path / "w")] + link)
    res = subprocess.run([str(tmp_path / "w")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr         # (without a GPU the constructor throws like the reference's: compile + link coverage)
    (tmp_path / "s.cpp").write_text(SHIM_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "mock_include"), "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / "s.cpp"), "-o", str(tmp_path / "s")] + link)


def test_demos_take_the_flag():
    assert '"--depth-filter"' in open(os.path.join(ROOT, "examples", "fp_demo.cpp")).read()
    assert '"--depth-filter"' in open(os.path.join(ROOT, "examples", "demo_sequence.py")).read()
    assert "--depth-filter)" in open(os.path.join(ROOT, "tools", "accept_real_assets.sh")).read()


# ---- plan_track_window --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def plan():
    L = _lib.test_lib()
    L.fpt_plan_track_window.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.fpt_plan_track_window.restype = None

    def ask(K, diameter, poses, H, W, reach):
        K = np.ascontiguousarray(K, np.float32)
        p16 = np.ascontiguousarray(syn.to_colmajor(np.asarray(poses, np.float32)))
        out = np.full((len(p16), 5), -7, np.int32)
        L.fpt_plan_track_window(K.ctypes.data, float(diameter), p16.ctypes.data, H, W, reach, out.ctypes.data, len(p16))
        return [tuple(int(v) for v in row) for row in out]
    return ask


def _poses(scenes, Wd, H):
    """the poses tests/test_nn_input_gpu.py tracks at: the perturbed ground truth, EDGE_T, BORDER_WINDOWS of this size; then drawn ones,
    from millimetres in front of the camera to 6 m, far off axis, behind the camera and with a translation of zero"""
    scene = scenes[Wd, H]
    out = [syn.perturb_pose(scene.gt_pose)]
    Rm = syn.random_rotation(11)
    out += [syn.pose_matrix(Rm, t) for t in EDGE_T]
    for w, h, ty in BORDER_WINDOWS:
        if (w, h) == (Wd, H):
            p = syn.perturb_pose(scene.gt_pose)
            p[1, 3] = ty
            out.append(p)
    rng = np.random.default_rng(Wd)
    for k in range(3000):
        tz = float(10.0 ** rng.uniform(-3, 0.8)) * (1 if k % 50 else -1)
        spread = (0.6, 3.0, 30.0)[k % 3]
        out.append(syn.pose_matrix(Rm, [rng.uniform(-spread, spread) * tz, rng.uniform(-spread, spread) * tz, tz]))
    out.append(syn.pose_matrix(Rm, [0, 0, 0]))
    out.append(syn.pose_matrix(Rm, [1e30, 0, 1e-5]))
    return np.stack(out).astype(np.float32)


@pytest.mark.parametrize("Wd,H", SIZES)
def test_window_plan_reach_0_is_the_estimate_track_made_before(plan, scenes, syn_mesh, Wd, H):
    scene = scenes[Wd, H]
    poses = _poses(scenes, Wd, H)
    got = plan(scene.K, syn_mesh.diameter, poses, H, Wd, 0)
    kinds = set()
    for p, g in zip(poses, got):
        want, _ = DC.window_before(scene.K, syn_mesh.diameter, p, H, Wd)
        kinds.add(want[0])
        if want[0] == DC.OUTSIDE:
            assert g[0] == DC.OUTSIDE and g[1] == g[2] == 0, (p[:3, 3], g, want)       # no row: nothing is uploaded, nothing read
        else:
            assert g == want, (p[:3, 3], g, want)
    assert kinds == {DC.WHOLE, DC.OUTSIDE, DC.ROWS, DC.RECT}                             # every outcome was asked for


@pytest.mark.parametrize("Wd,H", SIZES)
def test_window_plan_reach_4_grows_every_side_by_4_and_clamps(plan, scenes, syn_mesh, Wd, H):
    scene = scenes[Wd, H]
    poses = _poses(scenes, Wd, H)
    got0 = plan(scene.K, syn_mesh.diameter, poses, H, Wd, 0)
    got4 = plan(scene.K, syn_mesh.diameter, poses, H, Wd, 4)
    grown = clamped = 0
    for p, g0, g4 in zip(poses, got0, got4):
        (kind, *_), raw = DC.window_before(scene.K, syn_mesh.diameter, p, H, Wd)
        assert g4[0] == g0[0] == kind, (p[:3, 3], g0, g4)                                # the outcome does not depend on the reach
        if kind in (DC.WHOLE, DC.OUTSIDE):
            assert g4 == g0
            continue
        row0, row1, col0, col1 = raw
        want = DC.clamp(row0 - 4, row1 + 4, col0 - 4 if kind == DC.RECT else 0, col1 + 4 if kind == DC.RECT else -1, H, Wd)
        assert g4[1:] == want, (p[:3, 3], g4, want)
        # ... which is: every side of the reach-0 window 4 further out, unless the frame ends before
        assert g4[1] == max(g0[1] - 4, 0) or row0 < 0 and g4[1] == 0
        assert g4[2] == min(g0[2] + 4, H) or row1 > H and g4[2] == H
        assert 0 <= g4[1] <= g0[1] <= g0[2] <= g4[2] <= H and 0 <= g4[3] <= g0[3] <= g0[4] <= g4[4] <= Wd
        grown += g4[1] == g0[1] - 4 and g4[2] == g0[2] + 4 and (kind != DC.RECT or (g4[3] == g0[3] - 4 and g4[4] == g0[4] + 4))
        clamped += g4[1] == 0 or g4[2] == H or (kind == DC.RECT and (g4[3] == 0 or g4[4] == Wd))
    assert grown > 50 and clamped > 50


# ---- the GPU tests' inputs ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Wd,H", SIZES)
def test_the_filter_keeps_most_of_the_object_and_changes_it(scenes, syn_mesh, Wd, H):
    scene = scenes[Wd, H]
    p16 = syn.to_colmajor(syn.perturb_pose(scene.gt_pose)[None])
    filtered = fo.bilateral_filter_depth(fo.erode_depth(scene.depth))
    z_raw = fo.crop(scene.rgb, scene.depth, scene.K, p16, 1.2, syn_mesh.diameter)[0, :, :, 5]
    z_fil = fo.crop(scene.rgb, filtered, scene.K, p16, 1.2, syn_mesh.diameter)[0, :, :, 5]
    there = z_raw != 0
    assert there.sum() > 2000
    kept = float((z_fil[there] != 0).mean())
    differ = float((z_fil[there] != z_raw[there]).mean())
    print(f"{Wd}x{H}: the filtered crop keeps {kept:.3f} of {int(there.sum())} non-zero z pixels and differs on {differ:.3f} of them")
    assert kept >= 0.70 and differ > 0.5
