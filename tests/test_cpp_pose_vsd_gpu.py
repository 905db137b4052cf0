"""fp_amd::FoundationPose::PoseVsd (include/foundationpose_amd.hpp) compiles against the C-ABI library and returns the record of
tests/vsd_cases.py's "box_scaled" (every point of the box 1.5 times as far along its own ray: vsd exactly 1 and 0), which
tests/test_vsd_ref_cpu.py holds to its hand answer."""
import os
import subprocess

import numpy as np
import pytest

import vsd_cases as VC
from foundationpose_cpp_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include "foundationpose_amd.hpp"
int main() {
  fp_amd::Mesh m;
  m.name = "box";
  m.vertices = {%(vertices)s};
  m.normals = m.vertices;
  m.texcoords = std::vector<float>(16, 0.0f);
  m.faces = {%(faces)s};
  m.texture = std::vector<uint8_t>(12, 100);
  m.tex_height = 2; m.tex_width = 2; m.diameter = %(diameter)s;
  const float K[9] = {%(K)s};
  try {
    fp_amd::FoundationPose fp({m}, K, "", "");
    std::vector<uint8_t> rgb(%(H)d * %(W)d * 3, 0);
    std::vector<float> depth(%(H)d * %(W)d, 0.0f);
    if (fp_upload_frame(fp.handle(), rgb.data(), depth.data(), FP_HOST, %(H)d, %(W)d)) { std::printf("upload failed: %%s\n", fp_last_error()); return 2; }
    const fp_amd::Pose E = {%(E)s}, G = {%(G)s};
    std::vector<fp_pose_vsd_t> out;
    if (!fp.PoseVsd("box", {E, G}, {G}, out, 0.015f, {0.2f, 0.4f})) { std::printf("failed: %%s\n", fp.last_error().c_str()); return 2; }
    std::printf("scaled model=%%d/%%d inter=%%d union=%%d fail=%%d,%%d vsd=%%g,%%g status=%%d\n", out[0].n_model_est, out[0].n_model_gt, out[0].n_inter,
                out[0].n_union, out[0].n_fail[0], out[0].n_fail[1], out[0].vsd[0], out[0].vsd[1], out[0].status);
    std::printf("same inter=%%d union=%%d vsd=%%g,%%g\n", out[1].n_inter, out[1].n_union, out[1].vsd[0], out[1].vsd[1]);
    bool refused = !fp.PoseVsd("box", {E}, {G}, out, 0.015f, {});
    std::printf("no taus refused=%%d: %%s\n", (int)refused, fp.last_error().c_str());
    return refused ? 0 : 3;
  } catch (const std::runtime_error &e) {
    std::printf("threw: %%s\n", e.what());
    return 4;
  }
}
'''


def _floats(a):
    return ", ".join("%.9g" % x for x in np.asarray(a, np.float32).ravel())


def test_cpp_wrapper_pose_vsd(tmp_path):
    c = VC.case("box_scaled")
    mesh = VC.box()
    ref = VC.expected("box_scaled")[0]
    src = tmp_path / "t.cpp"
    src.write_text(SRC % dict(vertices=_floats(mesh.vertices), faces=", ".join(str(int(i)) for i in mesh.faces.ravel()),
                              diameter="%.9g" % np.float32(mesh.diameter), K=_floats(VC.K), H=VC.H, W=VC.W,
                              E=_floats(syn.to_colmajor(c["est"][0])), G=_floats(syn.to_colmajor(c["gt"][0]))))
    exe = tmp_path / "t"
    libdir = os.path.join(ROOT, "foundationpose_cpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lfoundationpose_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib"])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    n = ref["n_union"]
    assert n > 1500 and ref["n_fail"][:2] == [n, 0]
    assert f"scaled model={n}/{n} inter={n} union={n} fail={n},0 vsd=1,0 status=0" in lines, res.stdout
    assert f"same inter={n} union={n} vsd=0,0" in lines, res.stdout
    assert any(l.startswith("no taus refused=1") for l in lines), res.stdout
