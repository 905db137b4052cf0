"""fp_amd::FoundationPose::RefineDepth (include/foundationpose_amd.hpp) compiles against the C-ABI library and returns the hand answer of
tests/test_icp_ref_cpu.py: a plate facing the camera under a depth 3 mm behind it moves 3 mm along z, with rank 3, and with rank 1 when
only the translation is solved."""
import os
import subprocess

import numpy as np
import pytest

import frame_render_ref as FR
import icp_cases as IC
import icp_ref as IR
from foundationpose_cpp_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include "foundationpose_amd.hpp"
int main() {
  fp_amd::Mesh m;
  m.name = "plate";
  m.vertices = {%(vertices)s};
  m.normals = {0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1};
  m.texcoords = std::vector<float>(8, 0.0f);
  m.faces = {%(faces)s};
  m.texture = std::vector<uint8_t>(12, 100);
  m.tex_height = 2; m.tex_width = 2; m.diameter = %(diameter)s;
  const float K[9] = {%(K)s};
  try {
    fp_amd::FoundationPose fp({m}, K, "", "");
    std::vector<uint8_t> rgb(%(H)d * %(W)d * 3, 0);
    std::vector<float> depth(%(H)d * %(W)d, %(D)sf);
    if (fp_upload_frame(fp.handle(), rgb.data(), depth.data(), FP_HOST, %(H)d, %(W)d)) { std::printf("upload failed: %%s\n", fp_last_error()); return 2; }
    const fp_amd::Pose G = {%(G)s};
    std::vector<fp_amd::Pose> refined;
    std::vector<fp_depth_refine_t> out;
    if (!fp.RefineDepth("plate", {G, G}, refined, out, 0)) { std::printf("failed: %%s\n", fp.last_error().c_str()); return 2; }
    std::printf("measured used=%%d model=%%d iterations=%%d sum_e2=%%lld same=%%d\n", out[1].n_used, out[1].n_model, out[1].iterations,
                (long long)out[1].sums_q32[27], (int)(refined[1] == G));
    if (!fp.RefineDepth("plate", {G}, refined, out, 1)) { std::printf("failed: %%s\n", fp.last_error().c_str()); return 2; }
    std::printf("full rank=%%d iterations=%%d dz_um=%%.0f x_same=%%d\n", out[0].rank, out[0].iterations, (refined[0][14] - G[14]) * 1e6,
                (int)(refined[0][12] == G[12] && refined[0][13] == G[13]));
    if (!fp.RefineDepth("plate", {G}, refined, out, 1, 0.02f, true)) { std::printf("failed: %%s\n", fp.last_error().c_str()); return 2; }
    std::printf("translation rank=%%d dz_um=%%.0f\n", out[0].rank, (refined[0][14] - G[14]) * 1e6);
    bool refused = !fp.RefineDepth("plate", {G}, refined, out, 1, 1.0f);
    std::printf("gate above the diameter refused=%%d: %%s\n", (int)refused, fp.last_error().c_str());
    return refused ? 0 : 3;
  } catch (const std::runtime_error &e) {
    std::printf("threw: %%s\n", e.what());
    return 4;
  }
}
'''


def _floats(a):
    return ", ".join("%.9g" % x for x in np.asarray(a, np.float32).ravel())


def test_cpp_wrapper_refine_depth(tmp_path):
    mesh = IC.plate()
    ref = IR.sums(FR.centred(mesh), mesh.faces, IC.PLATE_G, IC.K, IC.PLATE_D, IC.GATE, mesh.diameter)
    src = tmp_path / "t.cpp"
    src.write_text(SRC % dict(vertices=_floats(mesh.vertices), faces=", ".join(str(int(i)) for i in mesh.faces.ravel()),
                              diameter="%.9g" % np.float32(mesh.diameter), K=_floats(IC.K), H=IC.H, W=IC.W, D="%.9g" % IC.PLATE_D[0, 0],
                              G=_floats(syn.to_colmajor(IC.PLATE_G))))
    exe = tmp_path / "t"
    libdir = os.path.join(ROOT, "foundationpose_cpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lfoundationpose_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib"])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    n = ref["n_used"]
    assert n == ref["n_model"] > 500
    assert f"measured used={n} model={n} iterations=0 sum_e2={ref['sums'][27]} same=1" in lines, res.stdout
    assert "full rank=3 iterations=1 dz_um=3000 x_same=1" in lines, res.stdout
    assert "translation rank=1 dz_um=3000" in lines, res.stdout
    assert any(l.startswith("gate above the diameter refused=1") and "max_dist_m" in l for l in lines), res.stdout
