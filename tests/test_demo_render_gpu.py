"""--render of the two demos (examples/demo_sequence.py, examples/fp_demo.cpp): with the flag off their output is byte for byte what it
is without it; with it on, <id>_render.png appears beside every box plot, holds the reference's overlay of the frame's pose, and the
poses and plots do not change."""
import os
import subprocess
import sys

import numpy as np
import pytest

import frame_render_ref as FR
from foundationpose_cpp_amd import dataset as D, load_mesh, synthetic as syn, weights as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def test_render_flag_of_both_demos(tmp_path):
    from PIL import Image
    root = str(tmp_path / "synthetic0")
    D.write_synthetic_sequence(root, n_frames=3)
    rp, sp = str(tmp_path / "r.fpw"), str(tmp_path / "s.fpw")
    W.pack_synthetic("refiner", rp)
    W.pack_synthetic("scorer", sp)
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import demo_sequence
    off, on = str(tmp_path / "py_off"), str(tmp_path / "py_on")
    poses_off = demo_sequence.run(root, rp, sp, off)
    poses_on = demo_sequence.run(root, rp, sp, on, render=True)
    assert np.array_equal(poses_off, poses_on)
    f_off, f_on = _files(off), _files(on)
    seq = D.Sequence(root)
    renders = {seq.ids[0] + "_render.png", seq.ids[-1] + "_render.png"}
    assert not [n for n in f_off if "render" in n] and set(f_on) == set(f_off) | renders
    assert all(f_on[n] == f_off[n] for n in f_off)
    # the picture is the reference's overlay of the pose the frame was given
    mesh = load_mesh("mustard", seq.mesh_path())
    for i in (0, len(seq) - 1):
        rgb, depth = seq.frame(i)
        ref = FR.render(FR.centred(mesh), mesh.faces, poses_on[i], seq.K, rgb, depth)
        img = np.asarray(Image.open(os.path.join(on, seq.ids[i] + "_render.png")))
        assert np.array_equal(img, ref["overlay"]) and (img != rgb).any(-1).sum() > 1000
    # the C++ demo writes the same files
    exe = str(tmp_path / "fp_demo")
    libdir = os.path.join(ROOT, "foundationpose_cpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "fp_demo.cpp"),
                           "-o", exe, "-L", libdir, "-lfoundationpose_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib"])
    c_off, c_on = str(tmp_path / "c_off"), str(tmp_path / "c_on")
    for out, extra in ((c_off, []), (c_on, ["--render"])):
        res = subprocess.run([exe, "--data", root, "--refiner", rp, "--scorer", sp, "--out", out] + extra, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout + res.stderr
    g_off, g_on = _files(c_off), _files(c_on)
    assert set(g_on) == set(g_off) | renders and all(g_on[n] == g_off[n] for n in g_off)
    for n in renders:
        assert np.array_equal(np.asarray(Image.open(os.path.join(c_on, n))), np.asarray(Image.open(os.path.join(on, n))))
