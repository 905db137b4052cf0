"""Cost of fp_pose_search and fp_register_depth on a geometry-only model of the 2 562-vertex ellipsoid in a
640 x 480 synthetic frame, at N = 252 and N = 1008 hypotheses (6 and 24 in-plane steps): one process, 2 warm-up calls then --calls timed
calls.  Per N: HIP-event time of the search kernel over the whole grid as fp_register_depth runs it (9 steps, 854 points; median, lowest,
highest), the wall time of that fp_pose_search call, the wall time of the whole fp_register_depth (sampler + search + ICP of 16
candidates, 15 iterations), and what it reaches against the scene's ground truth (MSSD over the ellipsoid's four equivalents).
   python tools/bench_depth_register.py [--calls 10]"""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch   # noqa: F401  before the library: both must share ONE HIP runtime
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foundationpose_cpp_amd import FoundationPose, synthetic as syn

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=10)
a = ap.parse_args()
WARM = 2


def stat(v, nd=4):
    return dict(median=round(statistics.median(v), nd), lo=round(min(v), nd), hi=round(max(v), nd))


mesh = syn.make_mesh()
scene = syn.make_scene(mesh)
m = FoundationPose(mesh, syn.intrinsics())
syms = np.stack([np.diag(np.array(d, np.float32)) for d in ((1, -1, -1, 1), (-1, 1, -1, 1), (-1, -1, 1, 1))])
vstep = (len(mesh.vertices) + 1023) // 1024
res = {"V": len(mesh.vertices), "points": -(-len(mesh.vertices) // vstep), "frame": list(scene.depth.shape)}
for steps in (6, 24):
    m.set_inplane_steps(steps)
    N = m.num_hypotheses

    def register():
        ok, pose, rec = m.register_depth(scene.rgb, scene.depth, scene.mask, mesh.name)
        assert ok, m.last_error
        return pose, rec

    for _ in range(WARM):
        pose, rec = register()
    hyp = m.get_hyp_poses(scene.mask)
    for _ in range(WARM):
        m.pose_search(mesh.name, hyp, vertex_step=vstep)
    wall, wall_search, kernel = [], [], []
    for _ in range(a.calls):
        t0 = time.perf_counter(); pose, rec = register(); wall.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); m.pose_search(mesh.name, hyp, vertex_step=vstep); wall_search.append((time.perf_counter() - t0) * 1e3)
    for _ in range(a.calls):
        m.profile_reset(); m.profile(True)
        m.pose_search(mesh.name, hyp, vertex_step=vstep)
        rep = m.profile_report(); m.profile(False)
        kernel.append(rep["pose_search"]["ms"])
    err = m.pose_errors(mesh.name, [pose], scene.gt_pose, symmetries=syms, adds=False)[0]
    res[f"N{N}"] = {"pose_search_kernel_ms": stat(kernel), "pose_search_call_wall_ms": stat(wall_search, 3), "register_depth_wall_ms": stat(wall, 3),
                    "point_tests": N * 9 * res["points"], "hypothesis": rec.hypothesis, "rank_key": rec.rank_key, "n_used": rec.refine.n_used,
                    "icp_updates": rec.refine.iterations, "mssd_mm": round(err.mssd_m * 1e3, 4), "rot_deg": round(err.rot_deg, 4)}
m.close()
print(json.dumps(res))
