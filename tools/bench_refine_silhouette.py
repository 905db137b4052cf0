"""Cost of fp_refine_silhouette on a geometry-only model of the 10 242-vertex icosphere in a 640 x 480 synthetic
frame with the scene's own mask -- the workload of tools/bench_pose_silhouette.py: N = 1 / 252 poses, --iterations updates; one process, 2
warm-up calls then --calls timed calls.  Per N: wall time of the call without the profiler (median, lowest, highest) and per evaluation,
HIP-event time of the five kernel families, the faces the call's (pose, tile) items walk over its evaluations and faces / second of
silref_tile -- the figure FP_SILREF_MAX_WORK is set from -- and, in the same run, alternating call by call, fp_refine_depth over the
same poses and iteration count (icp_tile walks the same items).  No target is set.
   python tools/bench_refine_silhouette.py [--calls 10] [--iterations 4]"""
import argparse, ctypes as C, json, os, statistics, sys, time
import numpy as np
import torch   # before the library: both must share ONE HIP runtime  # noqa: F401
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foundationpose_cpp_amd import FoundationPose, _lib, synthetic as syn
from foundationpose_cpp_amd.api import _p

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--iterations", type=int, default=4)
a = ap.parse_args()
WARM = 2


def stat(v, nd=4):
    return dict(median=round(statistics.median(v), nd), lo=round(min(v), nd), hi=round(max(v), nd))


mesh = syn.make_mesh(subdiv=5)
scene = syn.make_scene(mesh)
H, W = scene.depth.shape
mask = np.ascontiguousarray(scene.mask, np.uint8)
m = FoundationPose(mesh, syn.intrinsics())
m.upload_frame(scene.rgb, scene.depth)
gt = np.asarray(scene.gt_pose, np.float32)
F = len(mesh.faces)


def profiled(fn, families):
    ms, calls = {k: [] for k in families}, {}
    for _ in range(a.calls):
        m.profile_reset(); m.profile(True)
        fn()
        rep = m.profile_report(); m.profile(False)
        for k in families:
            ms[k].append(rep[k]["ms"])
            calls[k] = rep[k]["calls"]
    out = {k + "_ms": stat(x) for k, x in ms.items()}
    out["launches"] = calls
    return out


def walled(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


res = {"V": len(mesh.vertices), "F": F, "frame": [H, W], "n_mask": int((mask > 0).sum()), "iterations": a.iterations}
for N in (1, 252):
    poses = np.stack([syn.perturb_pose(gt, deg=3.0 + 0.1 * i, trans=0.005 + 0.0001 * i, seed=i) for i in range(N)])
    est = syn.to_colmajor(poses)
    out_p, out = np.zeros_like(est), (_lib.FpSilhouetteRefine * N)()
    icp_p, icp_out = np.zeros_like(est), (_lib.FpDepthRefine * N)()

    def silhouette():
        m._must(m._L.fp_refine_silhouette(m._h, mesh.name.encode(), _p(mask), 0, _p(est), N, a.iterations, 0, 0.005, 0, _p(out_p), out))

    def depth():
        m._must(m._L.fp_refine_depth(m._h, mesh.name.encode(), _p(est), N, a.iterations, 0.02, 0, _p(icp_p), icp_out))

    for _ in range(WARM):
        silhouette(); depth()
    wall, base = [], []
    for _ in range(a.calls):                      # alternating: both see the same machine
        wall.append(walled(silhouette))
        base.append(walled(depth))
    r = profiled(silhouette, ("mask_edt_cols", "mask_edt_rows", "mask_signed_d2", "silref_vertex", "silref_tile"))
    evals = r["launches"]["silref_vertex"]        # (one chunk: a launch of the vertex pass per evaluation)
    r.update({"refine_depth_" + k: v for k, v in profiled(depth, ("icp_vertex", "icp_tile")).items()})
    r["call_wall_ms"] = stat(wall, 3)
    r["evaluations"] = evals
    r["wall_per_evaluation_ms"] = round(r["call_wall_ms"]["median"] / evals, 4)
    r["refine_depth_wall_ms"] = stat(base, 3)
    r["refine_depth_evaluations"] = r["refine_depth_launches"]["icp_vertex"]
    r["updates_first_last"] = [out[0].iterations, out[N - 1].iterations]
    r["rms_px_first"] = round(float(out[0].rms_px), 4)
    res[f"N{N}"] = r
# the faces walked by the last call (N = 252), evaluation by evaluation, as the library counts its items: the test build exports the bound
TL = _lib.test_lib()
TL.fpt_frame_tile_bound.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p]
v = mesh.vertices.astype(np.float32) - np.asarray(mesh.center, np.float32)
radius = float(np.float32(np.sqrt((v.astype(np.float64) ** 2).sum(1).max()) * (1.0 + 1e-6)))
K9 = np.ascontiguousarray(syn.intrinsics(), np.float32)


def tiles(p16):
    b = np.zeros(4, np.int32)
    TL.fpt_frame_tile_bound(_p(np.ascontiguousarray(p16, np.float32)), _p(K9), radius, H, W, _p(b))
    return 0 if b[0] > b[2] or b[1] > b[3] else int(b[2] - b[0] + 1) * int(b[3] - b[1] + 1)


# (the poses move by a few pixels at most: the items of an evaluation are counted at the input poses and at the returned ones, and the
# mean of the two stands for every evaluation)
r = res["N252"]
items = 0.5 * (sum(tiles(p) for p in est) + sum(tiles(p) for p in out_p))
r["items_per_evaluation"] = items
r["faces_walked"] = items * F * r["evaluations"]
r["silref_faces_per_s"] = float("%.4g" % (r["faces_walked"] / (r["silref_tile_ms"]["median"] * 1e-3)))
r["icp_faces_per_s"] = float("%.4g" % (items * F * r["refine_depth_evaluations"] / (r["refine_depth_icp_tile_ms"]["median"] * 1e-3)))
r["silref_over_icp"] = round(r["silref_faces_per_s"] / r["icp_faces_per_s"], 3)
m.close()
print(json.dumps(res))
