"""Cost of fp_pose_vsd on a geometry-only model of the 10 242-vertex icosphere in a 640 x 480 synthetic frame:
N = 1 / 42 / 252 estimates against one truth (n_gt == 1), BOP19's ten thresholds; one process, 2 warm-up calls then --calls timed calls.
Per N: wall time of the call without the profiler (median, lowest, highest), HIP-event time of the two kernel families, the faces the
call's (pose, tile) items walk and their rate, faces / second of vsd_tile -- the figure FP_VSD_MAX_WORK is set from -- and, in the same
run, the baseline a caller had before the call existed: N + 1 fp_render_pose calls with only model_depth, FP_DEVICE (nothing is read
back and nothing compared: the baseline is the cheaper half of the job).  The two alternate call by call.
   python tools/bench_pose_vsd.py [--calls 10]"""
import argparse, ctypes as C, json, os, statistics, sys, time
import numpy as np
import torch   # before the library: both must share ONE HIP runtime
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foundationpose_cpp_amd import BOP19_TAUS, FoundationPose, _lib, synthetic as syn
from foundationpose_cpp_amd.api import FP_DEVICE, _p

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=10)
a = ap.parse_args()
WARM = 2
FAMILIES = ("vsd_vertex", "vsd_tile")
TILE = 32


def stat(v, nd=4):
    return dict(median=round(statistics.median(v), nd), lo=round(min(v), nd), hi=round(max(v), nd))


mesh = syn.make_mesh(subdiv=5)
scene = syn.make_scene(mesh)
H, W = scene.depth.shape
m = FoundationPose(mesh, syn.intrinsics())
m.upload_frame(scene.rgb, scene.depth)
gt = np.asarray(scene.gt_pose, np.float32)
taus = np.asarray(BOP19_TAUS, np.float32)
plane = torch.zeros((H, W), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
only_depth = _lib.FpFrameRender(model_depth=C.c_void_p(plane.data_ptr()))

# the tiles of a pose's screen bound, as the library forms them (the test build exports the function)
TL = _lib.test_lib()
TL.fpt_frame_tile_bound.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p]
v = mesh.vertices.astype(np.float32) - np.asarray(mesh.center, np.float32)
radius = float(np.float32(np.sqrt((v.astype(np.float64) ** 2).sum(1).max()) * (1.0 + 1e-6)))
K9 = np.ascontiguousarray(syn.intrinsics(), np.float32)


def bound(p16):
    out = np.zeros(4, np.int32)
    TL.fpt_frame_tile_bound(_p(p16), _p(K9), radius, H, W, _p(out))
    return out


def tiles(b):
    return 0 if b[0] > b[2] or b[1] > b[3] else int(b[2] - b[0] + 1) * int(b[3] - b[1] + 1)


res = {"V": len(mesh.vertices), "F": len(mesh.faces), "frame": [H, W]}
for N in (1, 42, 252):
    est = syn.to_colmajor(np.stack([syn.perturb_pose(gt, deg=3.0 + 0.1 * i, trans=0.005 + 0.0001 * i, seed=i) for i in range(N)]))
    g16 = syn.to_colmajor(gt[None])
    out = (_lib.FpPoseVsd * N)()
    bg = bound(g16[0])
    items = 0
    for p in est:
        be = bound(p)
        items += tiles([min(be[0], bg[0]), min(be[1], bg[1]), max(be[2], bg[2]), max(be[3], bg[3])])
    work = (items + tiles(bg)) * len(mesh.faces)

    def vsd():
        m._must(m._L.fp_pose_vsd(m._h, mesh.name.encode(), _p(est), N, _p(g16), 1, 0.015, _p(taus), len(taus), 1, out))

    def baseline():
        for p in list(est) + [g16[0]]:
            m._must(m._L.fp_render_pose(m._h, mesh.name.encode(), _p(np.ascontiguousarray(p)), 0.005, C.byref(only_depth), FP_DEVICE))

    for _ in range(WARM):
        vsd(); baseline()
    wall, base = [], []
    for _ in range(a.calls):                      # alternating: both see the same machine
        t0 = time.perf_counter(); vsd(); wall.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); baseline(); base.append((time.perf_counter() - t0) * 1e3)
    ms = {k: [] for k in FAMILIES}
    for _ in range(a.calls):
        m.profile_reset(); m.profile(True)
        vsd()
        rep = m.profile_report(); m.profile(False)
        for k in FAMILIES:
            ms[k].append(rep[k]["ms"])
    r = {k + "_ms": stat(x) for k, x in ms.items()}
    r["call_wall_ms"] = stat(wall, 3)
    r["baseline_render_pose_wall_ms"] = stat(base, 3)
    r["items"] = items
    r["faces_walked"] = work
    r["faces_per_s"] = float("%.4g" % (work / (r["vsd_tile_ms"]["median"] * 1e-3)))
    r["vsd_first"] = [round(float(x), 4) for x in out[0].vsd[:len(taus)]]
    r["n_union_first"] = out[0].n_union
    res[f"N{N}"] = r
m.close()
print(json.dumps(res))
