"""Cost of fp_pose_color on a geometry-only model of the 10 242-vertex icosphere in a 640 x 480 synthetic frame --
the workload of tools/bench_pose_vsd.py: N = 1 / 252 poses; one process, 2 warm-up calls then --calls timed calls.  Per N: wall time of the
call without the profiler (median, lowest, highest), HIP-event time of the two kernel families, the faces the call's (pose, tile) items
walk and faces / second of color_tile -- the figure FP_COLOR_MAX_WORK is set from -- and, in the same run and on the same poses, the
yardstick: icp_tile of one evaluation of fp_refine_depth (iterations = 0), whose items and walk are the same.  The two alternate call by
call.  Then the zncc a caller may expect (the tests assert no constant): the true pose and its three equivalents on that frame, and the
pose fp_register_depth returns on a frame WITHOUT the object (a wall at 1.5 m, a picture of noise) in the 200 x 150 scene of the tests.
   python tools/bench_pose_color.py [--calls 10]"""
import argparse, ctypes as C, json, os, statistics, sys, time
import numpy as np
import torch   # before the library: both must share ONE HIP runtime  # noqa: F401
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foundationpose_cpp_amd import FoundationPose, _lib, synthetic as syn
from foundationpose_cpp_amd.api import _p

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=10)
a = ap.parse_args()
WARM = 2


def stat(v, nd=4):
    return dict(median=round(statistics.median(v), nd), lo=round(min(v), nd), hi=round(max(v), nd))


mesh = syn.make_mesh(subdiv=5)
scene = syn.make_scene(mesh)
H, W = scene.depth.shape
m = FoundationPose(mesh, syn.intrinsics())
m.upload_frame(scene.rgb, scene.depth)
gt = np.asarray(scene.gt_pose, np.float32)

# the tiles of a pose's screen bound, as the library forms them (the test build exports the function)
TL = _lib.test_lib()
TL.fpt_frame_tile_bound.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p]
v = mesh.vertices.astype(np.float32) - np.asarray(mesh.center, np.float32)
radius = float(np.float32(np.sqrt((v.astype(np.float64) ** 2).sum(1).max()) * (1.0 + 1e-6)))
K9 = np.ascontiguousarray(syn.intrinsics(), np.float32)


def tiles(p16):
    b = np.zeros(4, np.int32)
    TL.fpt_frame_tile_bound(_p(p16), _p(K9), radius, H, W, _p(b))
    return 0 if b[0] > b[2] or b[1] > b[3] else int(b[2] - b[0] + 1) * int(b[3] - b[1] + 1)


def profiled(fn, families):
    ms = {k: [] for k in families}
    for _ in range(a.calls):
        m.profile_reset(); m.profile(True)
        fn()
        rep = m.profile_report(); m.profile(False)
        for k in families:
            ms[k].append(rep[k]["ms"])
    return {k + "_ms": stat(x) for k, x in ms.items()}


res = {"V": len(mesh.vertices), "F": len(mesh.faces), "frame": [H, W]}
for N in (1, 252):
    est = syn.to_colmajor(np.stack([syn.perturb_pose(gt, deg=3.0 + 0.1 * i, trans=0.005 + 0.0001 * i, seed=i) for i in range(N)]))
    out = (_lib.FpPoseColor * N)()
    icp_out, icp_poses = (_lib.FpDepthRefine * N)(), np.zeros_like(est)
    items = sum(tiles(p) for p in est)
    work = items * len(mesh.faces)

    def color():
        m._must(m._L.fp_pose_color(m._h, mesh.name.encode(), _p(est), N, 0.005, out))

    def icp():
        m._must(m._L.fp_refine_depth(m._h, mesh.name.encode(), _p(est), N, 0, 0.02, 0, _p(icp_poses), icp_out))

    for _ in range(WARM):
        color(); icp()
    wall, base = [], []
    for _ in range(a.calls):                      # alternating: both see the same machine
        t0 = time.perf_counter(); color(); wall.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); icp(); base.append((time.perf_counter() - t0) * 1e3)
    r = profiled(color, ("color_vertex", "color_tile"))
    r.update(profiled(icp, ("icp_vertex", "icp_tile")))
    r["call_wall_ms"] = stat(wall, 3)
    r["refine_depth_0_iterations_wall_ms"] = stat(base, 3)
    r["items"] = items
    r["faces_walked"] = work
    r["color_faces_per_s"] = float("%.4g" % (work / (r["color_tile_ms"]["median"] * 1e-3)))
    r["icp_faces_per_s"] = float("%.4g" % (work / (r["icp_tile_ms"]["median"] * 1e-3)))
    r["color_over_icp"] = round(r["color_faces_per_s"] / r["icp_faces_per_s"], 3)
    r["zncc_first"] = round(float(out[0].zncc), 4)
    r["n_compared_first"] = out[0].n_compared
    res[f"N{N}"] = r

# what the zncc is: the truth and its equivalents on this frame ...
eq = [gt] + [gt @ np.diag(np.array(d + (1,), np.float32)) for d in ((1, -1, -1), (-1, 1, -1), (-1, -1, 1))]
res["zncc_truth_and_equivalents"] = [round(r.zncc, 4) for r in m.pose_color(mesh.name, eq)]
m.close()
# ... and where the object is not there: the tests' 200 x 150 scene, a wall at 1.5 m, a picture of noise
small = syn.make_mesh(subdiv=3)
sw, sh = 200, 150
sc = syn.make_scene(small, W=sw, H=sh, t=(0.01, -0.005, 0.35), rot_seed=1, noise_seed=2, drop_seed=3, bg_seed=4)
m = FoundationPose(small, syn.intrinsics(sw, sh))
ok, pose, rec = m.register_depth(sc.rgb, sc.depth, sc.mask, small.name)
assert ok, m.last_error
res["scene_200x150"] = {"rank_key": rec.rank_key, "zncc_of_the_equivalents": [round(r.zncc, 4) for r in m.pose_color(
    small.name, [pose] + [pose @ np.diag(np.array(d + (1,), np.float32)) for d in ((1, -1, -1), (-1, 1, -1), (-1, -1, 1))])]}
noise = np.random.default_rng(4).integers(0, 256, (sh, sw, 3)).astype(np.uint8)
ok, pose, rec = m.register_depth(noise, np.full((sh, sw), np.float32(1.5)), sc.mask, small.name, top_k=4, icp_iterations=5)
if ok:
    r = m.pose_color(small.name, [pose])[0]
    res["wall_only_200x150"] = {"rank_key": rec.rank_key, "n_compared": r.n_compared, "status": r.status, "zncc": round(r.zncc, 4)}
else:
    res["wall_only_200x150"] = {"failed": m.last_error}
m.close()
print(json.dumps(res))
