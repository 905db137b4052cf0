"""Cost of fp_render_scene at 1280x720 with DEVICE outputs, one process, 5 warm-up calls then --calls timed calls:
  (a) K = 8 copies of the 5 120-triangle icosphere spread over the frame, against eight sequential fp_render_pose calls (all five outputs
      each, device memory) in the same process.  GATE: the median wall time of the one scene call is below the median of the eight calls
      together (exit status 1 otherwise).
  (b) K = 1 with the 81 920-triangle icosphere against fp_render_pose at the same pose: what binning does to the triangle walk.  No gate.
Per case: wall time of the call(s) without the profiler, then HIP-event time per profiled kernel family (median, lowest, highest).
   python tools/bench_render_scene.py [--calls 30]"""
import argparse, ctypes as C, json, os, statistics, sys, time
import numpy as np
import torch   # before the library: both must share ONE HIP runtime
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foundationpose_cpp_amd import FoundationPose, _lib, synthetic as syn
from foundationpose_cpp_amd.api import FP_DEVICE, _p

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
a = ap.parse_args()
W, H = 1280, 720
WARM = 5


def stat(v, nd=4):
    return dict(median=round(statistics.median(v), nd), lo=round(min(v), nd), hi=round(max(v), nd))


def dev(*shape):
    return torch.zeros(shape, dtype=torch.uint8, device="cuda")


def measure(m, call, families):
    """-> wall ms per call (profiler off) and ms per kernel family per call (profiler on)"""
    for _ in range(WARM):
        call()
    wall = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    ms = {k: [] for k in families}
    for _ in range(a.calls):
        m.profile_reset(); m.profile(True)
        call()
        rep = m.profile_report(); m.profile(False)
        for k in families:
            ms[k].append(rep[k]["ms"])
    out = {k + "_ms": stat(v) for k, v in ms.items()}
    out["kernels_ms"] = stat([sum(ms[k][i] for k in families) for i in range(a.calls)])
    out["call_wall_ms"] = stat(wall, 3)
    return out


def run(sub, poses):
    mesh = syn.make_mesh(subdiv=sub)
    scene = syn.make_scene(mesh, W=W, H=H)
    m = FoundationPose(mesh, scene.K)
    rgb_d, depth_d = torch.from_numpy(scene.rgb).cuda(), torch.from_numpy(scene.depth).cuda()
    bufs = dict(model_depth=dev(H, W, 4), instance_id=dev(H, W), visible_mask=dev(H, W), tri_id=dev(H, W, 4), cover_bits=dev(H, W, 8),
                overlay=dev(H, W, 3), model_mask=dev(H, W))
    torch.cuda.synchronize()
    m._must(m._L.fp_upload_frame(m._h, C.c_void_p(rgb_d.data_ptr()), C.c_void_p(depth_d.data_ptr()), FP_DEVICE, H, W))
    K = len(poses)
    p16 = syn.to_colmajor(np.asarray(poses, np.float32))
    names = (C.c_char_p * K)(*[mesh.name.encode()] * K)
    srec = _lib.FpSceneRender(**{n: C.c_void_p(bufs[n].data_ptr()) for n in ("model_depth", "instance_id", "visible_mask", "tri_id", "cover_bits", "overlay")})
    prec = _lib.FpFrameRender(**{n: C.c_void_p(bufs[n].data_ptr()) for n in ("model_depth", "model_mask", "visible_mask", "tri_id", "overlay")})
    recs = (_lib.FpSceneObject * K)()

    def scene_call():
        m._must(m._L.fp_render_scene(m._h, K, names, _p(p16), 0.005, C.byref(srec), recs, FP_DEVICE))

    def pose_calls():
        for o in range(K):
            m._must(m._L.fp_render_pose(m._h, mesh.name.encode(), _p(p16[o]), 0.005, C.byref(prec), FP_DEVICE))

    out = dict(faces_per_object=len(mesh.faces), K=K)
    out["render_scene"] = measure(m, scene_call, ("scene_vertex", "scene_bin", "scene_raster"))
    out["render_scene"]["n_covered"] = [r.n_covered for r in recs]
    out["render_pose_x%d" % K] = measure(m, pose_calls, ("frame_vertex", "frame_raster"))
    torch.cuda.synchronize()
    m.close()
    return out


gt = syn.make_scene(syn.make_mesh(1), W=W, H=H).gt_pose
eight = []
for i in range(8):
    r, c = divmod(i, 4)
    p = syn.pose_matrix(syn.random_rotation(20 + i), ((c - 1.5) * 0.25, (r - 0.5) * 0.3, 0.7))
    eight.append(p)
res = {"a_K8_F5120": run(4, eight), "b_K1_F81920": run(6, [gt])}
one, many = res["a_K8_F5120"]["render_scene"]["call_wall_ms"]["median"], res["a_K8_F5120"]["render_pose_x8"]["call_wall_ms"]["median"]
res["gate_a_scene_wall_below_eight_pose_calls"] = bool(one < many)
print(json.dumps(res))
sys.exit(0 if one < many else 1)
