"""Cost of fp_render_pose at 1280x720 with icospheres of 5 k and 82 k triangles (the sizes tools/mesh_size_sweep.py
uses): HIP-event time of the two profiled kernel families per call, warm, median with the spread over the calls, next to the bytes the
raster kernel reads and writes; and the host wall time of the whole call (vertex pass, flag read-back, raster, five device -> host copies,
one synchronisation).   python tools/bench_render_pose.py [--calls 30] [--subdiv 4 6]"""
import argparse, json, os, statistics, sys, time
import torch   # before the library: both must share ONE HIP runtime
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foundationpose_cpp_amd import FoundationPose, synthetic as syn

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--subdiv", type=int, nargs="*", default=[4, 6])
a = ap.parse_args()
W, H = 1280, 720
out = {}
for sub in a.subdiv:
    mesh = syn.make_mesh(subdiv=sub)
    scene = syn.make_scene(mesh, W=W, H=H)
    m = FoundationPose(mesh, scene.K)
    m.upload_frame(scene.rgb, scene.depth)
    for want in (("model_depth", "model_mask", "visible_mask", "tri_id", "overlay"), ("visible_mask",)):
        for _ in range(5):
            r = m.render_pose(mesh.name, scene.gt_pose, want=want)
        ms = {"frame_vertex": [], "frame_raster": []}
        wall = []
        for _ in range(a.calls):
            m.profile_reset(); m.profile(True)
            t0 = time.perf_counter()
            m.render_pose(mesh.name, scene.gt_pose, want=want)
            wall.append((time.perf_counter() - t0) * 1e3)
            rep = m.profile_report(); m.profile(False)
            for k in ms:
                ms[k].append(rep[k]["ms"])
        nbytes = rep["frame_raster"]["bytes"]
        key = f"F{len(mesh.faces)}_{'all5' if len(want) == 5 else want[0]}"
        out[key] = {k + "_ms": dict(median=round(statistics.median(v), 4), lo=round(min(v), 4), hi=round(max(v), 4)) for k, v in ms.items()}
        out[key]["raster_frame_bytes"] = nbytes
        out[key]["call_wall_ms"] = dict(median=round(statistics.median(wall), 3), lo=round(min(wall), 3), hi=round(max(wall), 3))
        out[key]["model_px"] = int((r[want[-1]] > 0).sum()) if want[-1] != "overlay" else int((r["model_mask"] > 0).sum())
    m.close()
print(json.dumps(out))
