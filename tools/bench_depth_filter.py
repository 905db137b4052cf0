"""Cost of the depth filter option: a replayed Track from a host frame and from a device frame at 640x480 and
1280x720, and Register N = 252, with the option off and on, interleaved in one process, warm; the median of each round's median with the
spread over rounds (lo / hi).  A build without the option (an older checkout) is timed "off" only, for comparison on the same box:
    python tools/bench_depth_filter.py [--rounds 5]"""
import argparse, ctypes as C, json, os, statistics, sys, tempfile, time
import torch   # before the library: both must share ONE HIP runtime
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from foundationpose_cpp_amd import FoundationPose, synthetic as syn, weights as W
from foundationpose_cpp_amd.api import FP_DEVICE, _p

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
mesh = syn.make_mesh()
d = tempfile.mkdtemp(); rp, sp = os.path.join(d, "r.fpw"), os.path.join(d, "s.fpw")
W.pack_synthetic("refiner", rp); W.pack_synthetic("scorer", sp)
res = {}
for Wd, H in ((640, 480), (1280, 720)):
    scene = syn.make_scene(mesh, Wd, H)
    hyp = syn.perturb_pose(scene.gt_pose)
    m = FoundationPose(mesh, scene.K, rp, sp)
    has = hasattr(m, "set_depth_filter")
    r_d, d_d = torch.from_numpy(scene.rgb).cuda(), torch.from_numpy(scene.depth).cuda()
    p16, out = syn.to_colmajor(hyp[None])[0], np.zeros(16, np.float32)

    def track_device():
        return (m._L.fp_track_ex(m._h, C.c_void_p(r_d.data_ptr()), C.c_void_p(d_d.data_ptr()), FP_DEVICE, H, Wd, _p(p16), mesh.name.encode(), 1, _p(out)) == 0,)
    work = {"track_host_us": (lambda: m.Track(scene.rgb, scene.depth, hyp, mesh.name), 400, 1e6),
            "track_device_us": (track_device, 400, 1e6)}
    if Wd == 640:
        work["register252_ms"] = (lambda: m.Register(scene.rgb, scene.depth, scene.mask, mesh.name), 30, 1e3)

    def timed(fn, reps, scale):
        for _ in range(5):
            assert fn()[0], m.last_error        # eager, capture, replay, warm
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts) * scale
    for r in range(a.rounds):
        for on in ([False, True] if has else [False]):
            if has:
                m.set_depth_filter(on)
            for k, (fn, reps, scale) in work.items():
                res.setdefault(f"{Wd}x{H}.{k}.{'on' if on else 'off'}", []).append(timed(fn, reps, scale))
    m.close()
out = {k: dict(median=round(statistics.median(v), 3), lo=round(min(v), 3), hi=round(max(v), 3)) for k, v in res.items()}
for k in [k for k in out if k.endswith(".on")]:
    out[k[:-3] + ".cost"] = round(out[k]["median"] - out[k[:-3] + ".off"]["median"], 3)
print(json.dumps(out))
