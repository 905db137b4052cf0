"""Cost of fp_pose_errors on a geometry-only model of the 10 242-vertex icosphere: N = 1 / 252 poses at
Vs = 1025 (vertex_step 10) / 10 242 (vertex_step 1), no symmetries, with FP_POSE_ERROR_ADDS; one process, 2 warm-up calls then --calls
timed calls.  Per case: wall time of the call without the profiler, HIP-event time of the two kernel families (median, lowest, highest)
and the point pairs per second of the nearest-neighbour kernel, N * Vs^2 / its median time -- the figure FP_POSE_ERROR_MAX_PAIRS is set from.
Last, the paired kernel at scale: 252 poses x 1025 symmetries x 1025 vertices without ADD-S, in transformed vertex pairs per second.
   python tools/bench_pose_errors.py [--calls 10]"""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch   # before the library: both must share ONE HIP runtime
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foundationpose_cpp_amd import FoundationPose, _lib, synthetic as syn
from foundationpose_cpp_amd.api import _p

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=10)
a = ap.parse_args()
WARM = 2
FAMILIES = ("pose_error_pairs", "pose_error_nn")


def stat(v, nd=4):
    return dict(median=round(statistics.median(v), nd), lo=round(min(v), nd), hi=round(max(v), nd))


def measure(m, call):
    for _ in range(WARM):
        call()
    wall = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    ms = {k: [] for k in FAMILIES}
    for _ in range(a.calls):
        m.profile_reset(); m.profile(True)
        call()
        rep = m.profile_report(); m.profile(False)
        for k in FAMILIES:
            ms[k].append(rep[k]["ms"])
    out = {k + "_ms": stat(v) for k, v in ms.items()}
    out["call_wall_ms"] = stat(wall, 3)
    return out


mesh = syn.make_mesh(subdiv=5)
m = FoundationPose(mesh, syn.intrinsics())
gt = syn.pose_matrix(syn.random_rotation(1), (0.02, -0.01, 0.7))
res = {"V": len(mesh.vertices)}
for N in (1, 252):
    est = syn.to_colmajor(np.stack([syn.perturb_pose(gt, deg=3.0 + 0.1 * i, trans=0.005, seed=i) for i in range(N)]))
    g16 = syn.to_colmajor(gt[None])
    out = (_lib.FpPoseError * N)()
    for step in (10, 1):
        def call():
            m._must(m._L.fp_pose_errors(m._h, mesh.name.encode(), _p(est), N, _p(g16), 1, None, 0, step, 1, out))
        r = measure(m, call)
        Vs = out[0].n_vertices
        r["pairs"] = N * Vs * Vs
        r["nn_pairs_per_s"] = float("%.4g" % (r["pairs"] / (r["pose_error_nn_ms"]["median"] * 1e-3)))
        r["adds_mm_first"] = round(out[0].adds_m * 1e3, 4)
        res[f"N{N}_Vs{Vs}"] = r

# the paired kernel at scale: 252 poses x (1024 symmetries + identity) x 1025 vertices, without ADD-S
N, S, step = 252, 1024, 10
c = np.asarray(mesh.center, np.float64)
sym = np.tile(np.eye(4), (S, 1, 1))
for k in range(S):
    ang = 2 * np.pi * (k + 1) / (S + 1)
    sym[k, :3, :3] = [[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]
    sym[k, :3, 3] = c - sym[k, :3, :3] @ c
s16 = syn.to_colmajor(sym)
est = syn.to_colmajor(np.stack([syn.perturb_pose(gt, deg=3.0 + 0.1 * i, trans=0.005, seed=i) for i in range(N)]))
g16 = syn.to_colmajor(gt[None])
out = (_lib.FpPoseError * N)()


def paired():
    m._must(m._L.fp_pose_errors(m._h, mesh.name.encode(), _p(est), N, _p(g16), 1, _p(s16), S, step, 0, out))


FAMILIES = ("pose_error_pairs",)
r = measure(m, paired)
r["vertex_pairs"] = N * (S + 1) * out[0].n_vertices
r["vertex_pairs_per_s"] = float("%.4g" % (r["vertex_pairs"] / (r["pose_error_pairs_ms"]["median"] * 1e-3)))
res[f"paired_N{N}_S{S}_Vs{out[0].n_vertices}"] = r
m.close()
print(json.dumps(res))
