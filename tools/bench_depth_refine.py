"""Cost of fp_refine_depth on a geometry-only model of the 10 242-vertex icosphere in a 640 x 480 synthetic frame:
N = 1 and N = 252 poses, one process, 2 warm-up calls then --calls timed calls.  Per N, with iterations = 0 (exactly one evaluation, so
the (pose, tile) items are those of the input poses): HIP-event time of the two kernel families (median, lowest, highest), the faces the
items walk and faces / second of icp_tile -- the figure FP_ICP_MAX_WORK is set from; then the wall time of the call with iterations = 0
and with iterations = 10, and what the ten iterations reach against the scene's ground truth.
   python tools/bench_depth_refine.py [--calls 10]"""
import argparse, ctypes as C, json, os, statistics, sys, time
import numpy as np
import torch   # before the library: both must share ONE HIP runtime
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foundationpose_cpp_amd import FoundationPose, _lib, synthetic as syn
from foundationpose_cpp_amd.api import _p

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=10)
a = ap.parse_args()
WARM = 2
FAMILIES = ("icp_vertex", "icp_tile")
GATE = 0.02


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


def gap(P):
    c = (np.trace(P[:3, :3].astype(np.float64) @ gt[:3, :3].astype(np.float64).T) - 1) / 2
    return float(np.degrees(np.arccos(np.clip(c, -1, 1)))), float(np.linalg.norm(P[:3, 3].astype(np.float64) - gt[:3, 3]))


res = {"V": len(mesh.vertices), "F": len(mesh.faces), "frame": [H, W]}
for N in (1, 252):
    est = syn.to_colmajor(np.stack([syn.perturb_pose(gt, deg=3.0 + 0.02 * i, trans=0.005 + 0.00004 * i, seed=i) for i in range(N)]))
    out = (_lib.FpDepthRefine * N)()
    out_p = np.zeros((N, 16), np.float32)
    items = sum(tiles(p) for p in est)
    work = items * len(mesh.faces)

    def refine(iterations):
        m._must(m._L.fp_refine_depth(m._h, mesh.name.encode(), _p(est), N, iterations, GATE, 0, _p(out_p), out))

    for _ in range(WARM):
        refine(0); refine(10)
    wall0, wall10 = [], []
    for _ in range(a.calls):
        t0 = time.perf_counter(); refine(0); wall0.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); refine(10); wall10.append((time.perf_counter() - t0) * 1e3)
    ends = [gap(P) for P in syn.from_colmajor(out_p)]
    updates = [r.iterations for r in out]
    ms = {k: [] for k in FAMILIES}
    for _ in range(a.calls):
        m.profile_reset(); m.profile(True)
        refine(0)
        rep = m.profile_report(); m.profile(False)
        for k in FAMILIES:
            ms[k].append(rep[k]["ms"])
    r = {k + "_ms": stat(x) for k, x in ms.items()}
    r["call_wall_ms_0_iterations"] = stat(wall0, 3)
    r["call_wall_ms_10_iterations"] = stat(wall10, 3)
    r["items"] = items
    r["faces_walked"] = work
    r["faces_per_s"] = float("%.4g" % (work / (r["icp_tile_ms"]["median"] * 1e-3)))
    r["n_used_first"] = out[0].n_used
    r["updates"] = [min(updates), max(updates)]
    r["worst_deg_mm_after_10"] = [round(max(e[0] for e in ends), 4), round(max(e[1] for e in ends) * 1e3, 4)]
    res[f"N{N}"] = r
m.close()
print(json.dumps(res))
