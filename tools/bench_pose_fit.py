"""Cost of the pose fit: Track from host frames, fp_track_multi K = 8 and Register N = 252 with the option off and on,
interleaved in one process, warm, medians with the spread over rounds.  A build without the option (an older checkout) is timed "off" only,
for comparison on the same box:  python tools/bench_pose_fit.py [--rounds 5]"""
import argparse, json, os, statistics, sys, tempfile, time
import torch   # before the library: both must share ONE HIP runtime
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from foundationpose_cpp_amd import FoundationPose, synthetic as syn, weights as W

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
mesh = syn.make_mesh(); scene = syn.make_scene(mesh)
d = tempfile.mkdtemp(); rp, sp = os.path.join(d, "r.fpw"), os.path.join(d, "s.fpw")
W.pack_synthetic("refiner", rp); W.pack_synthetic("scorer", sp)
hyp = syn.perturb_pose(scene.gt_pose)
m = FoundationPose(mesh, scene.K, rp, sp)
has_fit = hasattr(m, "set_pose_fit")
hyps8, names8 = np.stack([hyp] * 8), [mesh.name] * 8
work = {"track_us": (lambda: m.Track(scene.rgb, scene.depth, hyp, mesh.name), 400, 1e6),
        "track_multi8_us": (lambda: m.track_multi(scene.rgb, scene.depth, hyps8, names8), 200, 1e6),
        "register252_ms": (lambda: m.Register(scene.rgb, scene.depth, scene.mask, mesh.name), 40, 1e3)}


def timed(fn, reps, scale):
    for _ in range(5):
        assert fn()[0], m.last_error        # eager, capture, replay, warm
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * scale


res = {}
for r in range(a.rounds):
    for on in ([False, True] if has_fit else [False]):
        if has_fit:
            m.set_pose_fit(on, 0.005)
        for k, (fn, reps, scale) in work.items():
            res.setdefault(f"{k}.{'on' if on else 'off'}", []).append(timed(fn, reps, scale))
out = {k: dict(median=round(statistics.median(v), 3), lo=round(min(v), 3), hi=round(max(v), 3)) for k, v in res.items()}
if has_fit:   # the kernel alone at N = 252 (Register's score pass): HIP-event time of the profiled family
    m.set_pose_fit(True, 0.005)
    ms = []
    for _ in range(10):
        m.profile_reset(); m.profile(True)
        m.Register(scene.rgb, scene.depth, scene.mask, mesh.name)
        rep = m.profile_report(); m.profile(False)
        ms.append(rep["pose_fit"]["ms"]); nbytes = rep["pose_fit"]["bytes"]
        crop = rep["crop_warp"]
    out["pose_fit_kernel_252"] = dict(ms=round(statistics.median(ms), 4), GBps=round(nbytes / statistics.median(ms) / 1e6, 1))
    out["crop_warp_profiled"] = dict(ms=round(crop["ms"], 4), calls=crop["calls"], GBps=round(crop["bytes"] / crop["ms"] / 1e6, 1))
print(json.dumps(out))
m.close()
