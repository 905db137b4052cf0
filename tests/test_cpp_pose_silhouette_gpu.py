"""fp_amd::FoundationPose::MaskDistance and PoseSilhouette (include/foundationpose_amd.hpp) compile against the C-ABI library and return
the record of tests/silhouette_cases.py's "hand_quad" (a two-triangle square half over a rectangular mask), which
tests/test_silhouette_ref_cpu.py holds to its hand answer."""
import os
import subprocess

import numpy as np
import pytest

import silhouette_cases as SIC
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
    for (int r = 60; r < 90; r++)
      for (int c = 100; c < 120; c++) mask[(size_t)r * W + c] = 255;
    if (fp_upload_frame(fp.handle(), rgb.data(), depth.data(), FP_HOST, H, W)) { std::printf("upload failed: %%s\n", fp_last_error()); return 2; }
    std::vector<uint32_t> to_mask, to_bg;
    if (!fp.MaskDistance(mask.data(), mask.size(), &to_mask, &to_bg)) { std::printf("failed: %%s\n", fp.last_error().c_str()); return 2; }
    unsigned long long t = 0;
    for (size_t i = 0; i < mask.size(); i++) if (mask[i]) t += to_bg[i];
    std::printf("distance sizes=%%d/%%d at(75,94)=%%u at(0,0)=%%u bg(75,100)=%%u bg(75,109)=%%u T=%%llu\n", (int)to_mask.size(), (int)to_bg.size(),
                to_mask[(size_t)75 * W + 94], to_mask[0], to_bg[(size_t)75 * W + 100], to_bg[(size_t)75 * W + 109], t);
    const fp_amd::Pose P = {%(P)s};
    std::vector<fp_pose_silhouette_t> out;
    for (int trunc : {0, 3}) {
      if (!fp.PoseSilhouette("quad", mask.data(), {P, P}, out, 0.005f, trunc)) { std::printf("failed: %%s\n", fp.last_error().c_str()); return 2; }
      std::printf("trunc=%%d n=%%d/%%d/%%d/%%d mask=%%d miss=%%d status=%%d spill=%%lld missed=%%lld iou=%%.9g rms=%%.9g/%%.9g\n", trunc, out[1].n_model,
                  out[1].n_visible, out[1].n_inter, out[1].n_spill, out[1].n_mask, out[1].n_miss, out[1].status, (long long)out[1].sum_spill_d2,
                  (long long)out[1].sum_miss_d2, out[1].iou, out[1].rms_spill_px, out[1].rms_miss_px);
    }
    bool refused = !fp.PoseSilhouette("nobody", mask.data(), {P}, out);
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


def test_cpp_wrappers_mask_distance_and_pose_silhouette(tmp_path):
    c = SIC.case("hand_quad")
    mesh = c["mesh"]
    assert c["D"].min() == c["D"].max() == np.float32(1.5) and (c["mask"] == SIC.hand_quad_mask()).all()
    assert np.abs(np.asarray(mesh.center)).max() == 0                      # the program leaves fp_amd::Mesh::center at its default of 0
    src = tmp_path / "t.cpp"
    src.write_text(SRC % dict(vertices=_floats(mesh.vertices), normals=_floats(mesh.normals), texcoords=_floats(mesh.texcoords),
                              texture=", ".join(str(int(x)) for x in mesh.texture.ravel()), diameter="%.9g" % np.float32(mesh.diameter),
                              K=_floats(SIC.K), H=SIC.H, W=SIC.W, P=_floats(syn.to_colmajor(c["poses"][0]))))
    exe = tmp_path / "t"
    libdir = os.path.join(ROOT, "foundationpose_cpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lfoundationpose_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib"])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    n = SIC.H * SIC.W
    # (75, 94) is 6 columns left of the mask; (0, 0) is 100 columns and 60 rows from its corner (60, 100)
    assert f"distance sizes={n}/{n} at(75,94)=36 at(0,0)={100 * 100 + 60 * 60} bg(75,100)=1 bg(75,109)=100 T=15840" in lines, res.stdout
    for trunc in (0, 3):
        r = SIC.hand_quad_expected(trunc)
        want = (f"trunc={trunc} n=144/144/72/72 mask=600 miss=528 status=0 spill={r['sum_spill_d2']} missed={r['sum_miss_d2']} "
                f"iou={'%.9g' % r['iou']} rms={'%.9g' % r['rms_spill_px']}/{'%.9g' % r['rms_miss_px']}")
        assert want in lines, (want, res.stdout)
    assert any(l.startswith("unknown refused=1") and "unknown target_name" in l for l in lines), res.stdout
