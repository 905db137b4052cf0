"""fp_amd::FoundationPose::RefineSilhouette (include/foundationpose_amd.hpp) compiles against the C-ABI library and returns the hand case
of tests/silref_cases.py (a two-triangle square against the same square two columns to the right), which tests/test_silref_ref_cpu.py
holds to its hand answer."""
import os
import subprocess

import numpy as np
import pytest

import silref_cases as SC
import silref_ref as RR
from foundationpose_cpp_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include "foundationpose_amd.hpp"
int main() {
  fp_amd::Mesh m;
  m.name = "quad";
  m.vertices = {%(vertices)s};
  m.normals = {%(normals)s};
  m.texcoords = {%(texcoords)s};
  m.faces = {0, 1, 2, 0, 2, 3};
  m.texture = {%(texture)s};
  m.tex_height = 2; m.tex_width = 2; m.diameter = %(diameter)s;
  const float K[9] = {%(K)s};
  try {
    fp_amd::FoundationPose fp({m}, K, "", "");
    const int H = %(H)d, W = %(W)d;
    std::vector<uint8_t> rgb((size_t)H * W * 3, 0), mask((size_t)H * W, 0);
    std::vector<float> depth((size_t)H * W, 1.5f);
    for (int r = 69; r < 81; r++)
      for (int c = 96; c < 108; c++) mask[(size_t)r * W + c] = 255;
    if (fp_upload_frame(fp.handle(), rgb.data(), depth.data(), FP_HOST, H, W)) { std::printf("upload failed: %%s\n", fp_last_error()); return 2; }
    const fp_amd::Pose P = {%(P)s};
    std::vector<fp_amd::Pose> refined;
    std::vector<fp_silhouette_refine_t> out;
    for (int iterations : {0, 2}) {
      if (!fp.RefineSilhouette("quad", mask.data(), {P, P}, refined, out, iterations, 0, 0.005f, FP_SILREF_TRANSLATION_ONLY)) {
        std::printf("failed: %%s\n", fp.last_error().c_str());
        return 2;
      }
      std::printf("iterations=%%d n=%%d/%%d/%%d/%%d/%%d/%%d/%%d done=%%d rank=%%d status=%%d e2=%%lld rms=%%.9g scale=%%.9g x=%%.4f\n", iterations, out[1].n_model,
                  out[1].n_contour, out[1].n_used, out[1].n_occluded, out[1].n_far, out[1].n_flat, out[1].n_steep, out[1].iterations, out[1].rank,
                  out[1].status, (long long)out[1].sums_q24[27], out[1].rms_px, out[1].scale_px, refined[1][12]);
    }
    bool refused = !fp.RefineSilhouette("nobody", mask.data(), {P}, refined, out);
    std::printf("unknown refused=%%d: %%s\n", (int)refused, fp.last_error().c_str());
    return refused ? 0 : 3;
  } catch (const std::runtime_error &e) {
    std::printf("threw: %%s\n", e.what());
    return 4;
  }
}
'''


def _floats(a):
    return ", ".join("%.9g" % x for x in np.asarray(a, np.float32).ravel())


def test_cpp_wrapper_refine_silhouette(tmp_path):
    c = SC.case("hand")
    mesh = c["mesh"]
    assert c["D"].min() == c["D"].max() == np.float32(1.5) and (c["mask"] == SC.hand_mask()).all()
    assert np.abs(np.asarray(mesh.center)).max() == 0                      # the program leaves fp_amd::Mesh::center at its default of 0
    src = tmp_path / "t.cpp"
    src.write_text(SRC % dict(vertices=_floats(mesh.vertices), normals=_floats(mesh.normals), texcoords=_floats(mesh.texcoords),
                              texture=", ".join(str(int(x)) for x in mesh.texture.ravel()), diameter="%.9g" % np.float32(mesh.diameter),
                              K=_floats(SC.K), H=SC.H, W=SC.W, P=_floats(syn.to_colmajor(c["poses"][0]))))
    exe = tmp_path / "t"
    libdir = os.path.join(ROOT, "foundationpose_cpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lfoundationpose_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib"])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    ev = SC.expected0("hand")[0]
    assert {k: ev[k] for k in RR.COUNTS} == SC.HAND
    want = (f"iterations=0 n=144/44/44/0/0/0/0 done=0 rank=0 status=0 e2={ev['sums'][27]} rms={'%.9g' % RR.rms_px(ev['sums'], 44, ev['scale_px'])} "
            f"scale={'%.9g' % ev['scale_px']} x=0.0000")
    assert want in lines, (want, res.stdout)
    two = [l for l in lines if l.startswith("iterations=2 ")]
    assert len(two) == 1 and " n=144/44/44/0/0/0/0 done=2 rank=3 status=0 e2=0 rms=0 " in two[0], res.stdout
    x = float(two[0].rsplit("x=", 1)[1])
    assert SC.HAND_STEP_X_M[0] - 0.002 <= x <= SC.HAND_STEP_X_M[1] + 0.002, x     # 2 px to the right, less what the second update takes back
    assert any(l.startswith("unknown refused=1") and "unknown target_name" in l for l in lines), res.stdout
