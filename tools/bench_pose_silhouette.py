"""Cost of fp_mask_distance and fp_pose_silhouette on a geometry-only model of the 10 242-vertex icosphere in a
640 x 480 synthetic frame with the scene's own mask -- the workload of tools/bench_pose_color.py: N = 1 / 252 poses; one process, 2 warm-up
calls then --calls timed calls.  Per N: wall time of the call without the profiler (median, lowest, highest), HIP-event time of the four
kernel families, the faces the call's (pose, tile) items walk and faces / second of silhouette_tile -- the figure FP_SIL_MAX_WORK is set
from -- and, in the same run and on the same poses, two yardsticks: color_tile of fp_pose_color, whose items and walk are the same (the
two alternate call by call), and the wall time of N calls of fp_render_pose (visible_mask only).  Then the wall time of
fp_mask_distance alone, and the IoU a caller may expect (the tests assert no constant): the truth and the truth moved sideways.
   python tools/bench_pose_silhouette.py [--calls 10]"""
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
mask = np.ascontiguousarray(scene.mask, np.uint8)
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


def walled(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


res = {"V": len(mesh.vertices), "F": len(mesh.faces), "frame": [H, W], "n_mask": int((mask > 0).sum())}
for N in (1, 252):
    poses = np.stack([syn.perturb_pose(gt, deg=3.0 + 0.1 * i, trans=0.005 + 0.0001 * i, seed=i) for i in range(N)])
    est = syn.to_colmajor(poses)
    out = (_lib.FpPoseSilhouette * N)()
    col_out = (_lib.FpPoseColor * N)()
    items = sum(tiles(p) for p in est)
    work = items * len(mesh.faces)

    def silhouette():
        m._must(m._L.fp_pose_silhouette(m._h, mesh.name.encode(), _p(mask), 0, _p(est), N, 0.005, 0, 0, out))

    def color():
        m._must(m._L.fp_pose_color(m._h, mesh.name.encode(), _p(est), N, 0.005, col_out))

    def renders():
        for P in poses:
            m.render_pose(mesh.name, P, want=("visible_mask",))

    for _ in range(WARM):
        silhouette(); color()
    wall, base = [], []
    for _ in range(a.calls):                      # alternating: both see the same machine
        wall.append(walled(silhouette))
        base.append(walled(color))
    r = profiled(silhouette, ("mask_edt_cols", "mask_edt_rows", "silhouette_vertex", "silhouette_tile"))
    r.update(profiled(color, ("color_vertex", "color_tile")))
    r["call_wall_ms"] = stat(wall, 3)
    r["pose_color_wall_ms"] = stat(base, 3)
    renders()
    r["render_pose_x_N_wall_ms"] = stat([walled(renders) for _ in range(3 if N > 1 else a.calls)], 3)
    r["items"] = items
    r["faces_walked"] = work
    r["silhouette_faces_per_s"] = float("%.4g" % (work / (r["silhouette_tile_ms"]["median"] * 1e-3)))
    r["color_faces_per_s"] = float("%.4g" % (work / (r["color_tile_ms"]["median"] * 1e-3)))
    r["silhouette_over_color"] = round(r["silhouette_faces_per_s"] / r["color_faces_per_s"], 3)
    r["iou_first"] = round(float(out[0].iou), 4)
    res[f"N{N}"] = r

a_map, b_map = np.zeros((H, W), np.uint32), np.zeros((H, W), np.uint32)


def distance():
    m._must(m._L.fp_mask_distance(m._h, _p(mask), 0, _p(a_map), _p(b_map)))


for _ in range(WARM):
    distance()
res["mask_distance_wall_ms"] = stat([walled(distance) for _ in range(a.calls)], 3)
res["largest_d2"] = [int(a_map.max()), int(b_map.max())]
# what the numbers are: the truth, and the truth moved sideways by 2, 5, 10, 20 mm
moved = [gt]
for mm in (2, 5, 10, 20):
    P = gt.copy()
    P[0, 3] += mm * 1e-3
    moved.append(P)
res["truth_and_moved_2_5_10_20_mm"] = [dict(iou=round(r.iou, 4), n_spill=r.n_spill, n_miss=r.n_miss, cost=r.sum_spill_d2 + r.sum_miss_d2)
                                       for r in m.pose_silhouette(mesh.name, mask, moved)]
m.close()
print(json.dumps(res))
