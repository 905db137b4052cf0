"""fp_amd::FoundationPose::PoseColor and ResolveSymmetry (include/foundationpose_amd.hpp) compile against the C-ABI library and return the
record of tests/color_cases.py's "hand_2x2" (one triangle seen head-on over a 2 x 2 texture), which tests/test_color_ref_cpu.py holds to
its hand answer."""
import os
import subprocess

import numpy as np
import pytest

import color_cases as CC
from foundationpose_cpp_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include "foundationpose_amd.hpp"
int main() {
  fp_amd::Mesh m;
  m.name = "hand";
  m.vertices = {%(vertices)s};
  m.normals = {%(normals)s};
  m.texcoords = {%(texcoords)s};
  m.faces = {0, 1, 2};
  m.texture = {%(texture)s};
  m.tex_height = 2; m.tex_width = 2; m.diameter = %(diameter)s;
  const float K[9] = {%(K)s};
  try {
    fp_amd::FoundationPose fp({m}, K, "", "");
    std::vector<uint8_t> rgb(%(H)d * %(W)d * 3);
    for (int r = 0; r < %(H)d; r++)
      for (int c = 0; c < %(W)d; c++)
        for (int ch = 0; ch < 3; ch++) rgb[((size_t)r * %(W)d + c) * 3 + ch] = (uint8_t)((3 * c + 5 * r + 7 * ch) %% 200);
    std::vector<float> depth(%(H)d * %(W)d, 1.5f);
    if (fp_upload_frame(fp.handle(), rgb.data(), depth.data(), FP_HOST, %(H)d, %(W)d)) { std::printf("upload failed: %%s\n", fp_last_error()); return 2; }
    const fp_amd::Pose P = {%(P)s};
    std::vector<fp_pose_color_t> out;
    if (!fp.PoseColor("hand", {P, P}, out)) { std::printf("failed: %%s\n", fp.last_error().c_str()); return 2; }
    std::printf("n=%%d/%%d/%%d/%%d status=%%d m=%%lld,%%lld,%%lld o=%%lld mm=%%lld oo=%%lld mo=%%lld,%%lld,%%lld zncc=%%.9g\n", out[1].n_model, out[1].n_visible,
                out[1].n_compared, out[1].n_nocolor, out[1].status, (long long)out[1].sum_m[0], (long long)out[1].sum_m[1], (long long)out[1].sum_m[2],
                (long long)out[1].sum_o[0], (long long)out[1].sum_mm[0], (long long)out[1].sum_oo[0], (long long)out[1].sum_mo[0],
                (long long)out[1].sum_mo[1], (long long)out[1].sum_mo[2], out[1].zncc);
    fp_amd::Pose back;
    int best = -1;
    std::vector<fp_pose_color_t> recs;
    if (!fp.ResolveSymmetry("hand", P, {}, back, &best, &recs)) { std::printf("failed: %%s\n", fp.last_error().c_str()); return 2; }
    std::printf("resolved best=%%d same=%%d records=%%d zncc=%%.9g\n", best, (int)(back == P), (int)recs.size(), recs[0].zncc);
    bool refused = !fp.PoseColor("nobody", {P}, out);
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


def test_cpp_wrappers_pose_color_and_resolve_symmetry(tmp_path):
    c = CC.case("hand_2x2")
    mesh = c["mesh"]
    ref = CC.hand_expected(2)
    assert mesh.texture.shape == (2, 2, 3) and c["D"].min() == c["D"].max() == np.float32(1.5) and (c["rgb"] == CC.hand_rgb()).all()
    assert np.abs(np.asarray(mesh.center)).max() == 0                      # the program leaves fp_amd::Mesh::center at its default of 0
    src = tmp_path / "t.cpp"
    src.write_text(SRC % dict(vertices=_floats(mesh.vertices), normals=_floats(mesh.normals), texcoords=_floats(mesh.texcoords),
                              texture=", ".join(str(int(x)) for x in mesh.texture.ravel()), diameter="%.9g" % np.float32(mesh.diameter),
                              K=_floats(CC.K), H=CC.H, W=CC.W, P=_floats(syn.to_colmajor(c["poses"][0]))))
    exe = tmp_path / "t"
    libdir = os.path.join(ROOT, "foundationpose_cpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lfoundationpose_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib"])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    z = "%.9g" % np.float32(ref["zncc"])
    want = (f"n=78/78/78/0 status=0 m={ref['sum_m'][0]},{ref['sum_m'][1]},{ref['sum_m'][2]} o={ref['sum_o'][0]} mm={ref['sum_mm'][0]} "
            f"oo={ref['sum_oo'][0]} mo={ref['sum_mo'][0]},{ref['sum_mo'][1]},{ref['sum_mo'][2]} zncc={z}")
    assert want in lines, (want, res.stdout)
    assert f"resolved best=0 same=1 records=1 zncc={z}" in lines, res.stdout
    assert any(l.startswith("unknown refused=1") and "unknown target_name" in l for l in lines), res.stdout
