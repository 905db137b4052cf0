"""Rasteriser time of a vertex-coloured mesh against its textured twin: Register (N = 252) on the synthetic mesh, the `raster_shade`
family of fp_profile_report, per Register (two launches: the refiner's pass at crop ratio 1.2, the scorer's at 1.1), several rounds so
that the run-to-run spread is on the page (EXPERIMENTS.md, "Vertex colours").   python tools/vertex_color_timing.py [rounds]"""
import dataclasses, os, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from foundationpose_cpp_amd import FoundationPose, synthetic as syn, weights as W
d = tempfile.mkdtemp(); rp, sp = os.path.join(d, "r.fpw"), os.path.join(d, "s.fpw")
W.pack_synthetic("refiner", rp); W.pack_synthetic("scorer", sp)
mesh = syn.make_mesh(); scene = syn.make_scene(mesh)
twin = dataclasses.replace(mesh, name="col", vertex_colors=np.random.default_rng(21).integers(0, 256, (len(mesh.vertices), 3), dtype=np.uint8))
twin.color_source = 1
m = FoundationPose([mesh, twin], scene.K, rp, sp)
rounds, n = (int(sys.argv[1]) if len(sys.argv) > 1 else 5), 8
res = {mesh.name: [], twin.name: []}
for name in res:
    for _ in range(2): m.Register(scene.rgb, scene.depth, scene.mask, name)
for r in range(rounds):
    for name in res:
        m.profile(True); m.profile_reset()
        for _ in range(n):
            ok, _ = m.Register(scene.rgb, scene.depth, scene.mask, name); assert ok, m.last_error
        rep = m.profile_report(); m.profile(False)
        res[name].append(rep["raster_shade"]["ms"] * 1e3 / n)
for name, v in res.items():
    print(f"{name:10s} raster_shade per Register (N = 252): median {np.median(v):.1f} us, min {min(v):.1f}, max {max(v):.1f}  ({', '.join('%.1f' % x for x in v)})")
m.close()
