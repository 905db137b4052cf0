"""fp_amd::FoundationPose::RegisterDepth and ::PoseSearch (include/foundationpose_amd.hpp) compile against the C-ABI library and return
what the C calls return: the same pose and record as fp_register_depth, which is also what the Python face gets on the same frame."""
import os
import subprocess

import numpy as np
import pytest

import icp_cases as IC
from foundationpose_cpp_amd import FoundationPose, synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include <cstring>
#include "foundationpose_amd.hpp"
template <class T> static std::vector<T> slurp(const char *path, size_t n) {
  std::vector<T> v(n);
  FILE *f = std::fopen(path, "rb");
  if (!f || std::fread(v.data(), sizeof(T), n, f) != n) { std::printf("cannot read %%s\n", path); std::exit(5); }
  std::fclose(f);
  return v;
}
int main(int argc, char **argv) {
  const int H = %(H)d, W = %(W)d, V = %(V)d, F = %(F)d;
  fp_amd::Mesh m;
  m.name = "ico2";
  m.vertices = slurp<float>(argv[1], (size_t)V * 3);
  m.normals = slurp<float>(argv[2], (size_t)V * 3);
  m.texcoords = std::vector<float>((size_t)V * 2, 0.0f);
  m.faces = slurp<uint32_t>(argv[3], (size_t)F * 3);
  m.texture = std::vector<uint8_t>(12, 100);
  m.tex_height = 2; m.tex_width = 2; m.diameter = %(diameter)s;
  const float K[9] = {%(K)s};
  try {
    fp_amd::FoundationPose fp({m}, K, "", "");
    const std::vector<float> depth = slurp<float>(argv[4], (size_t)H * W);
    const std::vector<uint8_t> mask = slurp<uint8_t>(argv[5], (size_t)H * W);
    const std::vector<uint8_t> rgb((size_t)H * W * 3, 0);
    fp_amd::Pose pose, c_pose;
    fp_depth_register_t rec, c_rec;
    if (!fp.RegisterDepth({rgb.data(), H, W, 3}, {depth.data(), H, W}, {mask.data(), H, W, 1}, "ico2", pose, &rec)) {
      std::printf("failed: %%s\n", fp.last_error().c_str());
      return 2;
    }
    if (fp_register_depth(fp.handle(), rgb.data(), depth.data(), mask.data(), FP_HOST, H, W, "ico2", 16, 0.005f, 15, c_pose.data(), &c_rec)) return 3;
    std::printf("same=%%d\n", (int)(pose == c_pose && std::memcmp(&rec, &c_rec, sizeof(rec)) == 0));
    std::printf("pose");
    for (float v : pose) std::printf(" %%.9g", v);
    std::printf("\nrecord hypothesis=%%d n=%%d candidates=%%d rank_key=%%d score=%%d n_used=%%d\n", rec.hypothesis, rec.n_hypotheses, rec.n_candidates,
                rec.rank_key, rec.search.score, rec.refine.n_used);
    std::vector<fp_pose_search_t> found;
    if (!fp.PoseSearch("ico2", {pose, pose}, found, 1, 0.0f)) { std::printf("failed: %%s\n", fp.last_error().c_str()); return 2; }
    std::printf("search n_points=%%d same=%%d inlier_share=%%d\n", found[1].n_points, (int)(std::memcmp(&found[0], &found[1], sizeof(found[0])) == 0),
                found[1].n_facing ? 100 * found[1].n_inlier / found[1].n_facing : 0);
    const std::vector<uint8_t> empty((size_t)H * W, 0);
    fp_amd::Pose untouched = pose;
    bool refused = !fp.RegisterDepth({rgb.data(), H, W, 3}, {depth.data(), H, W}, {empty.data(), H, W, 1}, "ico2", untouched);
    std::printf("empty mask refused=%%d untouched=%%d: %%s\n", (int)refused, (int)(untouched == pose), fp.last_error().c_str());
    return refused ? 0 : 3;
  } catch (const std::runtime_error &e) {
    std::printf("threw: %%s\n", e.what());
    return 4;
  }
}
'''


def test_cpp_wrapper_register_depth(tmp_path):
    mesh = IC.ico(2)
    D = IC.rendering(mesh, IC.ICO_G)
    mask = np.where(D != IC.WALL, 255, 0).astype(np.uint8)
    files = []
    for name, a, dt in (("v", mesh.vertices, np.float32), ("n", mesh.normals, np.float32), ("f", mesh.faces, np.uint32), ("d", D, np.float32),
                        ("m", mask, np.uint8)):
        files.append(str(tmp_path / name))
        np.ascontiguousarray(a, dt).tofile(files[-1])
    src = tmp_path / "t.cpp"
    src.write_text(SRC % dict(H=IC.H, W=IC.W, V=len(mesh.vertices), F=len(mesh.faces), diameter="%.9g" % np.float32(mesh.diameter),
                              K=", ".join("%.9g" % x for x in np.asarray(IC.K, np.float32).ravel())))
    exe = tmp_path / "t"
    libdir = os.path.join(ROOT, "foundationpose_cpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lfoundationpose_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib"])
    res = subprocess.run([str(exe)] + files, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    m = FoundationPose(mesh, IC.K)
    try:
        ok, pose, rec = m.register_depth(np.zeros((IC.H, IC.W, 3), np.uint8), D, mask, "ico2")
        assert ok, m.last_error
    finally:
        m.close()
    assert "same=1" in lines, res.stdout
    assert "pose " + " ".join("%.9g" % x for x in syn.to_colmajor(pose)) in lines, res.stdout
    assert (f"record hypothesis={rec.hypothesis} n=252 candidates=16 rank_key={rec.rank_key} score={rec.search.score} "
            f"n_used={rec.refine.n_used}") in lines, res.stdout
    found = [l for l in lines if l.startswith("search ")]
    assert found and found[0].startswith("search n_points=162 same=1 inlier_share=") and int(found[0].rsplit("=", 1)[1]) > 80, res.stdout
    assert any(l.startswith("empty mask refused=1 untouched=1") and "Mask is all zero" in l for l in lines), res.stdout
