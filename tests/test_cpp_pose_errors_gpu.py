"""fp_amd::FoundationPose::PoseErrors (include/foundationpose_amd.hpp) compiles against the C-ABI library and returns the hand answers of
tests/test_pose_error_ref_cpu.py for two points: every value below is exactly representable, so the comparison is exact."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cmath>
#include <cstdio>
#include "foundationpose_amd.hpp"
int main() {
  fp_amd::Mesh m;
  m.name = "pair";
  m.vertices = {-0.25f,0,0, 0.25f,0,0};
  m.normals = {0,0,-1, 0,0,-1};
  m.texcoords = {0,0, 1,0};
  m.faces = {0,0,0};
  m.texture = std::vector<uint8_t>(12, 100);
  m.tex_height = 2; m.tex_width = 2; m.diameter = 0.5f;
  const float K[9] = {320,0,320, 0,320,240, 0,0,1};
  try {
    fp_amd::FoundationPose fp({m}, K, "", "");
    const fp_amd::Pose E = {1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,2,1};
    const fp_amd::Pose moved = {1,0,0,0, 0,1,0,0, 0,0,1,0, 0.375f,0,2,1};
    const fp_amd::Pose flipped = {-1,0,0,0, 0,-1,0,0, 0,0,1,0, 0,0,2,1};
    const fp_amd::Pose flip = {-1,0,0,0, 0,-1,0,0, 0,0,1,0, 0,0,0,1};
    std::vector<fp_pose_error> out;
    if (!fp.PoseErrors("pair", {E, E}, {moved, flipped}, out)) { std::printf("failed: %s\n", fp.last_error().c_str()); return 2; }
    std::printf("moved add=%g adds=%g mssd=%g mspd=%g sym=%d trans=%g n=%d\n", out[0].add_m, out[0].adds_m, out[0].mssd_m, out[0].mspd_px,
                out[0].best_sym, out[0].trans_m, out[0].n_vertices);
    std::printf("flipped add=%g adds=%g mssd=%g sym=%d rot=%g\n", out[1].add_m, out[1].adds_m, out[1].mssd_m, out[1].best_sym, out[1].rot_deg);
    if (!fp.PoseErrors("pair", {E}, {flipped}, out, {flip}, 1, false)) { std::printf("failed: %s\n", fp.last_error().c_str()); return 2; }
    std::printf("symmetric add=%g adds_is_nan=%d mssd=%g mspd=%g sym=%d rot=%g\n", out[0].add_m, (int)std::isnan(out[0].adds_m), out[0].mssd_m,
                out[0].mspd_px, out[0].best_sym, out[0].rot_deg);
    bool refused = !fp.PoseErrors("pair", {E}, {E}, out, {}, 0);
    std::printf("vertex_step 0 refused=%d: %s\n", (int)refused, fp.last_error().c_str());
    return refused ? 0 : 3;
  } catch (const std::runtime_error &e) {
    std::printf("threw: %s\n", e.what());
    return 4;
  }
}
'''


def test_cpp_wrapper_pose_errors(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text(SRC)
    exe = tmp_path / "t"
    libdir = os.path.join(ROOT, "foundationpose_cpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lfoundationpose_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib"])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    assert "moved add=0.375 adds=0.25 mssd=0.375 mspd=60 sym=0 trans=0.375 n=2" in lines, res.stdout
    assert "flipped add=0.5 adds=0 mssd=0.5 sym=0 rot=180" in lines, res.stdout
    assert "symmetric add=0.5 adds_is_nan=1 mssd=0 mspd=0 sym=1 rot=0" in lines, res.stdout
    assert any(l.startswith("vertex_step 0 refused=1") and "vertex_step" in l for l in lines), res.stdout
