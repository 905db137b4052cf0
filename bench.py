#!/usr/bin/env python3
"""bench.py -- pose-hypotheses/sec of the Register hot path on MI355X (BASELINE.json metric).

A "step" is one Register over one batch of synthetic input (SURVEY.md §8d scene, 640x480, refine_itr = 1):
sampler -> render+crop (ratio 1.2) -> refine-net -> pose update -> render+crop (ratio 1.1) -> score-net -> arg-max,
with the frame (rgb, depth, mask) already resident in HBM when the timed region starts (`value`).  The same JSON line also
carries `host_frame` (the reference's calling convention: host frames, H2D inside the call) and `track` (Track fps, N = 1).

  N = 1  : workload = BASELINE.json configs[2] "Register, N=252 hypotheses, 640x480, single MI355X, fp16".
  N > 1  : one process per GPU -- `python bench.py --gpus N` spawns its own N ranks; under `python -m torch.distributed.run ...
           bench.py --gpus N` each process is one rank -- the SAME workload strong-scaled: BASELINE.json's metric is "Register
           N=252 ... at 1/2/4/8 GPUs": the 252 hypotheses are sharded in contiguous slices of ceil(252/N) per GPU, ONE RCCL
           all-gather of one row per hypothesis [pooled score feature 512 | pose 16] f32 -- issued by the LIBRARY on its own
           stream (fp_register_sharded) -- then every rank runs the cross-hypothesis attention + arg-max redundantly.  The ranks
           are torch-free: RCCL and HIP are /opt/rocm's through ctypes, the control plane (ncclUniqueId, barriers, max over ranks)
           is a localhost socket (foundationpose_cpp_amd/rendezvous.py).  Fewer devices than ranks is an error, never a smaller run.  The line also carries `n1008` = BASELINE configs[3] (1008
           hypotheses sharded the same way).  `--weak` keeps 252 hypotheses PER GPU (252*N in total) instead; `--hyps M` picks
           any total.

A plain run does only what the headline needs: set up, warm up, time the --steps steps, write --dump-outputs, print the JSON line.
`--full` adds everything else, all of it after the headline's timed region: the per-kernel profile step behind `roofline` and `stage_ms`,
the MFMA micro-benchmark, the CPU baseline, `n1008` (N > 1 as well) and these extra legs of the N = 1 run (a few steps each, every one
with its own roofline):
           `host_frame`, `track` (incl. pipelined / batched serving), `track_bf16` (configs[1]), `track_int8`, and configs[4] at 1280x720:
           `f16_720p`, `f16_720p_untextured` (the configs[4] path: f16) and the EXPERIMENTAL 8-bit legs `int8_720p`,
           `int8_720p_untextured` (8-bit trunk convolutions calibrated on 16 OTHER frames, measured on a held-out one, DISCRIMINATING synthetic
           weights; `--fp8-legs` adds the FP8 e4m3 pair) -- each 8-bit leg with an `accuracy` object: refined-pose deltas against the f16
           path, winner, teacher-forced rank, whether the 1 deg / 1 mm bar is met for >= 95 % of the hypotheses.

`--dump-outputs DIR` writes what the headline's last timed step handed its caller as DIR/<name>.npy: `pose` (4x4 row-major float32)
and, for N > 1, `winner` (the hypothesis index, float64).  The inputs are seeded, so two builds can be compared output for output.

Prints ONE JSON line on rank 0; with `--full` it carries two extra objects:
  roofline     -- dominant kernel (the conv/linear implicit-GEMM kernel with the largest share of the step, MFMA-bound):
                  algorithmic FLOPs of its launches in one step / their HIP-event durations on the library's stream
                  (fp_profile_*), vs the 2.5 PFLOP/s dense fp16 MFMA peak (and vs the rate a register-resident MFMA
                  micro-benchmark sustains on the same box, `peak_measured`); `traffic` = fabric bytes per launch from the
                  committed rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes (profiles/, corrected as the guide prescribes).
  cpu_baseline -- the oracle (C/OpenMP geometry + PyTorch-CPU fp32 networks), N = 8 Register, on the host cores.
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP16_TFLOPS = 2500.0   # MI355X dense fp16/bf16 MFMA peak (MI355X_MICROARCH.md)
PEAK_FP8_TFLOPS = 5000.0    # dense FP8 (v_mfma_f32_16x16x128_f8f6f4), same guide
PMC_FILE = "r06_register_n252_pmc_hbm.json"    # committed FETCH_SIZE / WRITE_SIZE passes of this round
STATS_FILE = "r06_register_n252_kernel_stats.csv"   # committed `rocprofv3 --kernel-trace --stats` summary of the same command
BASELINE_HYP_S = 705.6      # reference README.md:37-41: Register 2.8 fps x 252 on RTX 4060 (TensorRT fp16)


def cpu_baseline(mesh, scene, states, n_hyp=8, reps=8):
    """Register (refine_itr=1) over n_hyp hypotheses with the CPU oracle; returns hypotheses/s."""
    import torch
    from oracle import fp_oracle as fo
    from oracle import nets_torch as NT
    refiner, scorer = NT.build("refiner", states[0]), NT.build("scorer", states[1])
    om = fo.OracleMesh(mesh)
    threads = fo.num_threads()
    torch.set_num_threads(threads)
    t0 = time.perf_counter()
    for _ in range(reps):
        poses = fo.get_hyp_poses(scene.depth, scene.mask, scene.K)[:n_hyp]
        a = fo.render(om, poses, scene.K, scene.depth.shape, 1.2)
        b = fo.crop(scene.rgb, scene.depth, scene.K, poses, 1.2, mesh.diameter)
        with torch.no_grad():
            t, r = refiner(torch.from_numpy(a), torch.from_numpy(b))
        refined = fo.refine_post_process(poses, t.numpy(), r.numpy(), mesh.diameter)
        a = fo.render(om, refined, scene.K, scene.depth.shape, 1.1)
        b = fo.crop(scene.rgb, scene.depth, scene.K, refined, 1.1, mesh.diameter)
        with torch.no_grad():
            s = scorer(torch.from_numpy(a), torch.from_numpy(b)).numpy()
        fo.argmax(s)
    dt = time.perf_counter() - t0
    return dict(value=round(n_hyp * reps / dt, 3), unit="hypotheses/s", cores=threads, kind="port",
                sample=f"{reps} x Register N={n_hyp} 640x480 refine_itr=1 (oracle C/OpenMP geometry + PyTorch-CPU fp32 "
                       f"networks, {dt:.1f} s); the reference has no CPU path for this (SURVEY.md §8d)")


def dump_outputs(out_dir, **arrays):
    """--dump-outputs: one out_dir/<name>.npy per array (float32 / float64 only)."""
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(out_dir, f"{name}.npy"), a)

FP8_LAYERS = {"conv_128", "conv_256", "conv_b2", "conv_512"}   # 3x3 trunk convolutions from encodeA.2 on run on 8-bit operands in the fp8 / int8 modes
Q8 = ("fp8", "int8")
_Q8_TEXT = ("operands for the 13 3x3 trunk convolutions from encodeA.2 on (91 % of the FLOPs): per-output-channel weight scales, per-input-channel "
            "activation scales folded into the weights, f16 residual stream (dual-output epilogues), calibrated bias correction; f16 elsewhere")
_Q8_PMC = {"fp8": "r04", "int8": "r05c"}   # profiles/<tag>_register_<dtype>_720p_pmc_hbm.json
PRECISION_TEXT = {"f16": "f16 storage / f32 accumulate (the reference's TensorRT --fp16)", "bf16": "bf16 storage / f32 accumulate",
                  "fp8": "OCP e4m3 (v_mfma_f32_16x16x128_f8f6f4) " + _Q8_TEXT,
                  "int8": "8-bit integer (v_mfma_i32_16x16x64_i8; unsigned activations stored with an offset of -128) " + _Q8_TEXT}


def analyse_profile(prof, dtype, n_hyp, stages_per_hyp):
    """fp_profile_report of ONE step -> (roofline object of the dominant MFMA kernel, per-stage ms).
    Profiler keys are "<layer>/<kernel symbol>" for the conv family, "<kernel family>" otherwise."""
    conv = {k: v for k, v in prof.items() if k.startswith("conv_") or k.startswith("gemm_")}
    conv_flops = sum(v["flops"] for v in conv.values())
    conv_ms = sum(v["ms"] for v in conv.values())
    fp8_layers = FP8_LAYERS if dtype in Q8 else set()
    by_sym = {}
    for k, v in conv.items():
        layer = k.split("/", 1)[0]
        sym = k.split("/", 1)[1] if "/" in k else k
        if layer in fp8_layers and "halo8" not in sym:
            sym += f"[{dtype}]"
        a = by_sym.setdefault(sym, dict(ms=0.0, flops=0.0, bytes=0.0, calls=0, fp8=layer in fp8_layers))
        for f in ("ms", "flops", "bytes", "calls"):
            a[f] += v[f]
    dom, dv = max(by_sym.items(), key=lambda kv: kv[1]["ms"]) if by_sym else ("none", dict(ms=0, flops=0, bytes=0, calls=1, fp8=False))
    peak = PEAK_FP8_TFLOPS if dv.get("fp8") else PEAK_FP16_TFLOPS
    achieved = dv["flops"] / (dv["ms"] * 1e-3) / 1e12 if dv["ms"] > 0 else 0.0
    family = conv_flops / (conv_ms * 1e-3) / 1e12 if conv_ms > 0 else 0.0
    # the family's own ceiling: time at peak of every launch's FLOPs at its operand type
    ideal_ms = sum(v["flops"] / ((PEAK_FP8_TFLOPS if v["fp8"] else PEAK_FP16_TFLOPS) * 1e12) * 1e3 for v in by_sym.values())
    stages = {}
    for k, v in prof.items():
        stages[k.split("/", 1)[0]] = stages.get(k.split("/", 1)[0], 0.0) + v["ms"]
    # the HBM-bound sub-steps: vertex + raster/shade + observed-crop warp of every hypothesis-stage against
    # 0.9 MB per hypothesis-stage (fp16 network input written once + mesh + crop source window + texture taps)
    rc_ms = sum(stages.get(k, 0.0) for k in ("vertex", "raster_shade", "crop_warp"))
    n_stages = n_hyp * stages_per_hyp
    rc_gbs = n_stages * 0.9e6 / (rc_ms * 1e-3) / 1e9 if rc_ms > 0 else 0.0
    roof = {
        "bound": "mfma", "kernel": dom,
        "achieved": round(achieved, 1), "peak": peak, "unit": "TFLOP/s",
        "frac": round(achieved / peak, 4),
        "launches_per_step": dv["calls"], "algorithmic_gflop_per_launch": round(dv["flops"] / max(dv["calls"], 1) / 1e9, 1),
        "avg_launch_ms": round(dv["ms"] / max(dv["calls"], 1), 4),
        "algorithmic_bytes_per_launch": round(dv["bytes"] / max(dv["calls"], 1)),
        "conv_family": {"achieved": round(family, 1), "gflop_per_step": round(conv_flops / 1e9, 1), "ms_per_step": round(conv_ms, 3),
                        "ms_at_peak": round(ideal_ms, 3), "frac": round(ideal_ms / conv_ms, 4) if conv_ms > 0 else None,
                        "kernels_ms": {k2: round(v2["ms"], 3) for k2, v2 in by_sym.items()}},
        "render_crop": {"bound": "hbm", "achieved": round(rc_gbs, 1), "peak": 8000.0, "unit": "GB/s", "frac": round(rc_gbs / 8000.0, 4),
                        "ms_per_step": round(rc_ms, 4), "hypothesis_stages": n_stages,
                        "what": "vertex + raster_shade + crop_warp kernels, 0.9 MB algorithmic bytes per hypothesis-stage (SURVEY.md 8d)"},
    }
    stages = {k: round(v, 3) for k, v in sorted(stages.items(), key=lambda kv: -kv[1])}
    return roof, stages, dom, dv


# =====================================================================================================================================
# N > 1: one process per GPU.  The data plane is the LIBRARY's: fp_register_sharded issues the one ncclAllGather per Register on the
# model's own stream.  The control plane is foundationpose_cpp_amd/rendezvous.py (a localhost socket: the
# 128-byte ncclUniqueId, barriers, the max over ranks).  The ranks import neither torch nor a second HIP runtime: RCCL and HIP are
# /opt/rocm's, bound through ctypes -- the same runtime the library links.
# =====================================================================================================================================
def _hip_device_count():
    try:
        hip = C.CDLL("libamdhip64.so")
        n = C.c_int(0)
        return n.value if hip.hipGetDeviceCount(C.byref(n)) == 0 else 0
    except OSError:
        return 0


def launch_ranks(args):
    """`python bench.py --gpus N` without a launcher: spawn the N ranks (RANK / LOCAL_RANK / WORLD_SIZE set, HIP_VISIBLE_DEVICES untouched),
    serve the rendezvous from this process, relay their output, exit non-zero unless every rank succeeded."""
    import subprocess
    from foundationpose_cpp_amd import rendezvous
    n = args.gpus
    stub = os.environ.get("FP_BENCH_STUB_RANK") == "1"      # tests/test_bench_launcher_cpu.py: the launcher and control plane without a GPU
    have = n if stub else _hip_device_count()
    if have < n:
        print(f"bench.py: --gpus {n} needs {n} HIP devices, this box has {have}: refusing to run fewer ranks than asked for", file=sys.stderr)
        return 2
    server = rendezvous.Server(n)
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), FP_RDV_ADDR=server.address, HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    try:
        pending = set(range(n))
        while pending:
            for r in list(pending):
                code = procs[r].poll()
                if code is None:
                    continue
                pending.discard(r)
                if code != 0 and rc == 0:
                    rc = code if code > 0 else 1
                    print(f"bench.py: rank {r} exited with {code}; stopping the other ranks", file=sys.stderr)
                    for o in pending:
                        procs[o].terminate()          # the exact children started above
            time.sleep(0.05)
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    if rc == 0 and server.error is not None:
        print(f"bench.py: rendezvous server: {server.error}", file=sys.stderr)
        rc = 3
    return rc


class _NcclUniqueId(C.Structure):
    _fields_ = [("internal", C.c_char * 128)]


def rank_main(args, world):
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    stub = os.environ.get("FP_BENCH_STUB_RANK") == "1"
    assert "torch" not in sys.modules, "the rank processes are torch-free"
    from foundationpose_cpp_amd import rendezvous
    client, server = rendezvous.connect(rank, world)
    n_total = args.hyps if args.hyps > 0 else (252 * world if args.weak else 252)
    assert n_total % 42 == 0, "--hyps must be a multiple of 42 (icosphere views)"
    per = -(-n_total // world)

    def finish(res):
        sys.stdout.flush()
        try:
            C.CDLL(None).fflush(None)       # RCCL's banner goes through C stdio: out before the JSON line
        except OSError:
            pass
        client.barrier()
        if rank == 0:
            print(json.dumps(res), flush=True)
        client.barrier()
        client.close()
        if server is not None:
            server.join(5)
        return 0

    if stub:     # the control plane alone: every collective of the real body, no GPU work
        uid = client.broadcast(bytes(range(128)) if rank == 0 else None)
        assert uid == bytes(range(128))
        assert client.all_min_int(1) == 1
        client.barrier()
        t0 = time.perf_counter()
        time.sleep(0.01 * (rank + 1))
        dt = client.all_max(time.perf_counter() - t0)
        per_rank = client.gather_floats(0.01 * (rank + 1))
        winners = client.all_gather(str(7).encode())
        assert len(set(winners)) == 1
        return finish({"metric": f"pose-hypotheses/sec (Register N={n_total}, stub)", "value": round(n_total / dt, 2), "unit": "hypotheses/s", "n_gpus": world,
                       "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt * 1e3, 3), "higher_is_better": True, "scaling": "strong",
                       "vs_baseline": None, "dtype": args.dtype, "data": "stub", "config": {"workload": "launcher / control-plane stub (no GPU work)"},
                       "rccl_ranks_seen": len(per_rank), "per_rank_ms": [round(x * 1e3, 3) for x in per_rank]})

    # ---- RCCL first (RTLD_GLOBAL): the library binds "a copy already in the process" at its first sharded call
    err = None
    try:
        rccl = C.CDLL("librccl.so.1", mode=C.RTLD_GLOBAL)
        hip = C.CDLL("libamdhip64.so")
        ndev = C.c_int(0)
        if hip.hipGetDeviceCount(C.byref(ndev)) != 0 or ndev.value <= local_rank:
            err = f"rank {rank}: HIP device {local_rank} does not exist ({ndev.value} devices): --gpus {world} needs {world} GPUs"
        elif hip.hipSetDevice(local_rank) != 0:
            err = f"rank {rank}: hipSetDevice({local_rank}) failed"
    except OSError as e:
        err = f"rank {rank}: {e}"
    if client.all_min_int(0 if err else 1) == 0:      # every rank leaves together: nobody waits in a collective for a rank that never comes
        raise SystemExit(err or f"rank {rank}: another rank has no device; not running with fewer than {world} ranks")
    from foundationpose_cpp_amd import FoundationPose, synthetic as syn, weights as W
    from foundationpose_cpp_amd.api import FP_PREC_BF16
    if args.dtype not in ("f16", "bf16"):
        raise SystemExit("bench.py --gpus N > 1 runs the f16 / bf16 networks (the 8-bit precisions are single-GPU legs)")
    mesh = syn.make_mesh(textured=not args.untextured)
    scene = syn.make_scene(mesh, args.width, args.height)
    H, Wd = scene.depth.shape
    wdir = tempfile.mkdtemp()
    import atexit, shutil
    atexit.register(shutil.rmtree, wdir, True)
    rp, sp = os.path.join(wdir, "r.fpw"), os.path.join(wdir, "s.fpw")
    W.pack_synthetic("refiner", rp)
    W.pack_synthetic("scorer", sp)
    model = FoundationPose(mesh, scene.K, rp, sp, max_input_image_height=max(1080, args.height), max_input_image_width=max(1920, args.width), device=local_rank)
    if args.dtype == "bf16":
        model.set_precision(FP_PREC_BF16)
    model.set_inplane_steps(n_total // 42)

    # the frame resident in HBM (value's definition): device buffers of the runtime the library itself uses
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def to_device(a):
        a = np.ascontiguousarray(a)
        d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), a.nbytes) == 0 and hip.hipMemcpy(d, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0, "hipMalloc / hipMemcpy failed"
        return d
    d_rgb, d_depth, d_mask = to_device(scene.rgb), to_device(scene.depth), to_device(scene.mask)

    # ---- the communicator: rank 0 draws the id, the rendezvous carries its 128 bytes
    rccl.ncclGetUniqueId.argtypes = [C.POINTER(_NcclUniqueId)]
    rccl.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, _NcclUniqueId, C.c_int]
    rccl.ncclCommCount.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    rccl.ncclCommDestroy.argtypes = [C.c_void_p]
    rccl.ncclGetErrorString.restype = C.c_char_p
    uid = _NcclUniqueId()
    ok = 1
    if rank == 0:
        ok = 1 if rccl.ncclGetUniqueId(C.byref(uid)) == 0 else 0
    raw = client.broadcast(bytes(uid) if rank == 0 and ok else None)
    if len(raw) != 128:
        raise SystemExit(f"rank {rank}: rank 0 could not draw a ncclUniqueId")
    C.memmove(C.byref(uid), raw, 128)
    comm = C.c_void_p()
    rc = rccl.ncclCommInitRank(C.byref(comm), world, uid, rank)
    if client.all_min_int(1 if rc == 0 else 0) == 0:
        raise SystemExit(f"rank {rank}: ncclCommInitRank: {rccl.ncclGetErrorString(rc).decode() if rc else 'failed on another rank'}")
    seen = C.c_int(0)
    rccl.ncclCommCount(comm, C.byref(seen))

    out_pose = np.zeros(16, np.float32)
    idx = C.c_int(-1)

    def step():
        model._must(model._L.fp_register_sharded(model.handle, comm, d_rgb, d_depth, d_mask, 1, H, Wd, mesh.name.encode(), 1,
                                                 out_pose.ctypes.data_as(C.c_void_p), C.byref(idx)))

    def barrier():
        client.barrier()
        hip.hipDeviceSynchronize()

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        barrier()
        return time.perf_counter() - t0

    dt_own = timed(step, args.steps, args.warmup)
    dt = client.all_max(dt_own)                              # the job is as slow as its slowest rank
    per_rank_ms = client.gather_floats(dt_own / args.steps * 1e3)
    winners = [int(x) for x in client.all_gather(str(idx.value).encode())]
    poses = client.all_gather(out_pose.tobytes())
    if len(set(winners)) != 1 or len(set(poses)) != 1:
        raise SystemExit(f"rank {rank}: the ranks disagree on the winner / pose ({winners}): the redundant finish must be bit-identical")
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, pose=syn.from_colmajor(out_pose), winner=np.array([idx.value], np.float64))
    prof = None
    if args.full:                 # per-kernel-family event timing of ONE extra step
        model.profile(True)
        model.profile_reset()
        step()
        prof = model.profile_report()
        model.profile(False)
    n1008 = None
    if args.full and not args.no_extras and args.hyps == 0 and not args.weak:      # BASELINE configs[3]: 1008 hypotheses sharded the same way
        model.set_inplane_steps(24)
        k8 = max(3, args.steps // 4)
        t8 = client.all_max(timed(step, k8, 1))
        model.set_inplane_steps(n_total // 42)
        n1008 = {"metric": f"pose-hypotheses/sec (Register N=1008, {Wd}x{H})", "value": round(1008 * k8 / t8, 2), "unit": "hypotheses/s",
                 "ms_per_step": round(t8 / k8 * 1e3, 3), "steps": k8, "n_gpus": world, "scaling": "strong",
                 "workload": f"BASELINE configs[3]: Register N=1008 sharded, {-(-1008 // world)}/GPU, {Wd}x{H}, refine_itr=1, {args.dtype}"}
    res = None
    if rank == 0:
        res = {
            "metric": f"pose-hypotheses/sec (Register N={n_total}, {Wd}x{H})", "value": round(n_total * args.steps / dt, 2), "unit": "hypotheses/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "weak" if args.weak and args.hyps == 0 else "strong",
            "vs_baseline": round(n_total * args.steps / dt / BASELINE_HYP_S, 3), "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"Register N={n_total} hypotheses sharded, {per}/GPU, {Wd}x{H} refine_itr=1, frame resident in HBM",
                       "mesh": f"synthetic ellipsoid V=2562 F=5120, {'2x2 grey (untextured)' if args.untextured else '512x512 texture'}",
                       "weights": "synthetic (seed 7)", "precision": PRECISION_TEXT[args.dtype], "calibration": None,
                       "parallelism": f"hyp-shard x{world}: contiguous slices of {per} hypotheses, one process per GPU",
                       "collective": "1 ncclAllGather [n_local,528] f32 per Register, issued by the library on its own stream (fp_register_sharded); "
                                     "control plane: localhost socket rendezvous (ncclUniqueId, barriers, max over ranks), no torch in the ranks",
                       "baseline": "reference README.md:37-41 Register 2.8 fps x 252 = 705.6 hyp/s on RTX 4060 (TensorRT fp16)"},
            "rccl_ranks_seen": int(seen.value), "per_rank_ms": [round(x, 3) for x in per_rank_ms], "winner": winners[0],
        }
        if prof is not None:
            roof, stages, dom, dv = analyse_profile(prof, args.dtype, min(per, n_total), 2)
            res["roofline"] = dict(roof, what=f"rank 0's slice of {min(per, n_total)} hypotheses")
            res["stage_ms"] = stages
        if n1008 is not None:
            res["n1008"] = n1008
    model.close()
    rccl.ncclCommDestroy(comm)
    return finish(res)



def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hyps", type=int, default=0, help="total hypotheses sharded over the GPUs (default 252 = the BASELINE metric, strong scaling)")
    ap.add_argument("--weak", action="store_true", help="weak scaling: 252 hypotheses PER GPU (252*N in total)")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--dtype", choices=["f16", "bf16", "fp8", "int8"], default="f16",
                    help="network precision: f16 = the reference's TensorRT --fp16 engines (headline); bf16 = BASELINE configs[1]; "
                         "fp8 / int8 = 8-bit trunk convolutions (e4m3 / integers), BASELINE configs[4] (use with --width 1280 --height 720)")
    ap.add_argument("--untextured", action="store_true", help="the reference's 2x2 grey fallback texture (configs[4])")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure everything else: per-kernel profile and roofline, MFMA micro-benchmark, CPU baseline, "
                         "the extra legs (host frames, Track, n1008, the other BASELINE configs)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-mfma-peak", action="store_true", help="with --full: skip the MFMA micro-benchmark (profiling runs)")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the host-frame, Track and n1008 legs (profiling runs)")
    ap.add_argument("--fp8-legs", action="store_true", help="with --full: also run the two FP8 e4m3 720p legs (experimental: the precision fails the configs[4] parity bar)")
    ap.add_argument("--track", action="store_true", help="measure Track fps (N=1 hypothesis) as the headline instead of Register")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the headline's last timed step returned as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.fp8_legs and not args.full:
        ap.error("--fp8-legs adds legs to a --full run")

    # ---- who am I?  (contract: `python bench.py --gpus N` alone, or one rank of `python -m torch.distributed.run ... bench.py --gpus N`)
    world_env = os.environ.get("WORLD_SIZE")
    if args.gpus > 1 and world_env is None:
        sys.exit(launch_ranks(args))            # spawn the N ranks ourselves; rank 0 prints the JSON line
    world = int(world_env or "1")
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU (or run `python bench.py --gpus {args.gpus}` "
                         "without a launcher, it spawns its own ranks)")
    if world > 1 or os.environ.get("FP_BENCH_FORCE_SHARD", "0") == "1":
        sys.exit(rank_main(args, world))        # torch-free: RCCL + HIP through ctypes, control plane = foundationpose_cpp_amd/rendezvous.py

    import torch
    from foundationpose_cpp_amd import FoundationPose, synthetic as syn, weights as W
    from foundationpose_cpp_amd.api import FP_PREC_BF16, FP_PREC_F16, FP_PREC_FP8, FP_PREC_INT8
    Q8_PREC = {"fp8": FP_PREC_FP8, "int8": FP_PREC_INT8}

    rank, local_rank = 0, 0      # (the single-GPU body: N > 1 and FP_BENCH_FORCE_SHARD left through rank_main above)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP library has no CPU path")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    mesh = syn.make_mesh(textured=not args.untextured)
    scene = syn.make_scene(mesh, args.width, args.height)
    wdir = tempfile.mkdtemp()     # (kept until exit: the pipelined-Track leg creates more models from the same files)
    import atexit, shutil
    atexit.register(shutil.rmtree, wdir, True)
    rp_keep, sp_keep = os.path.join(wdir, f"r{rank}.fpw"), os.path.join(wdir, f"s{rank}.fpw")
    if True:
        d = wdir
        rp, sp = rp_keep, sp_keep
        states = (W.pack_synthetic("refiner", rp), W.pack_synthetic("scorer", sp))
        model = FoundationPose(mesh, scene.K, rp, sp, max_input_image_height=max(1080, args.height),
                               max_input_image_width=max(1920, args.width))
        if args.dtype in Q8:         # post-training static quantisation on 16 OTHER scenes (stated in config.calibration)
            model.calibrate_frames(syn.calibration_scenes(mesh, 16, W=args.width, H=args.height), mesh.name, Q8_PREC[args.dtype])
            model.set_precision(Q8_PREC[args.dtype])
        elif args.dtype == "bf16":
            model.set_precision(FP_PREC_BF16)

    n_total = args.hyps if args.hyps > 0 else (252 * world if args.weak else 252)
    assert n_total % 42 == 0, "--hyps must be a multiple of 42 (icosphere views)"
    model.set_inplane_steps(n_total // 42)
    rgb = torch.from_numpy(scene.rgb).to(dev)
    depth = torch.from_numpy(scene.depth).to(dev)
    mask = torch.from_numpy(scene.mask).to(dev)
    H, Wd = scene.depth.shape
    out_pose = np.zeros(16, np.float32)
    hyp16 = syn.to_colmajor(syn.perturb_pose(scene.gt_pose))
    hyp44 = syn.perturb_pose(scene.gt_pose)

    def track_dev():
        model._must(model._L.fp_track_ex(model.handle, C.c_void_p(rgb.data_ptr()), C.c_void_p(depth.data_ptr()), 1,
                                         H, Wd, hyp16.ctypes.data_as(C.c_void_p), mesh.name.encode(), 1,
                                         out_pose.ctypes.data_as(C.c_void_p)))

    def register_dev():
        model._must(model._L.fp_register_ex(model.handle, C.c_void_p(rgb.data_ptr()), C.c_void_p(depth.data_ptr()),
                                            C.c_void_p(mask.data_ptr()), 1, H, Wd, mesh.name.encode(), 1,
                                            out_pose.ctypes.data_as(C.c_void_p)))

    def step():
        if args.track:
            track_dev()
        else:
            register_dev()

    def barrier():
        torch.cuda.synchronize()

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        barrier()
        return time.perf_counter() - t0

    dt = timed(step, args.steps, args.warmup)
    if args.dump_outputs:         # now: every later leg reuses out_pose
        dump_outputs(args.dump_outputs, pose=syn.from_colmajor(out_pose))

    # ---- --full from here on: nothing below feeds the headline
    # per-kernel-family event timing of ONE extra step (outside the timed region)
    if args.full:
        model.profile(True)
        model.profile_reset()
        step()
        prof = model.profile_report()
        model.profile(False)

    # ---- extra legs on one GPU (outside the headline's timed region): the reference's calling convention (host frames,
    # H2D inside the call: speed_register / speed_track, simple_tests/src/test_foundationpose.cpp:118-127,145-154) and Track
    extras = {}
    if args.full and not args.no_extras:
        def register_host():
            ok, _ = model.Register(scene.rgb, scene.depth, scene.mask, mesh.name)
            assert ok, model.last_error

        def track_host():
            ok, _ = model.Track(scene.rgb, scene.depth, hyp44, mesh.name)
            assert ok, model.last_error

        if not args.track:
            th = timed(register_host, args.steps, 2)
            extras["host_frame"] = {
                "value": round(n_total * args.steps / th, 2), "unit": "hypotheses/s", "ms_per_step": round(th / args.steps * 1e3, 3),
                "what": "fp_register from pageable host frames: H2D of rgb + depth + mask inside the timed call (the reference's "
                        "speed_register convention); `value` above is the same call with the frame resident in HBM"}
        ksteps = max(args.steps * 10, 100)
        td = timed(track_dev, ksteps, 10)
        thh = timed(track_host, ksteps, 10)
        model.profile(True)
        model.profile_reset()
        track_dev()
        tprof = model.profile_report()
        model.profile(False)
        tconv = {k: v for k, v in tprof.items() if k.startswith("conv_") or k.startswith("gemm_")}
        tflops = sum(v["flops"] for v in tconv.values()) + sum(v["flops"] for k, v in tprof.items() if k == "attention")
        # pipelined serving: ONE host thread keeps K models (objects of one scene, frame resident in HBM) in flight with
        # fp_track_submit / fp_track_wait -- Track is launch-latency-bound, so independent objects overlap on the chip
        pipelined = None
        if args.dtype == "f16":
            K_OBJ = 8
            others = [FoundationPose(mesh, scene.K, rp_keep, sp_keep, max_input_image_height=max(1080, args.height),
                                     max_input_image_width=max(1920, args.width)) for _ in range(K_OBJ - 1)]
            fleet = [model] + others
            outs = np.zeros(16, np.float32)

            def submit_all():
                for mm in fleet:
                    mm._must(mm._L.fp_track_submit(mm.handle, C.c_void_p(rgb.data_ptr()), C.c_void_p(depth.data_ptr()), 1, H, Wd,
                                                   hyp16.ctypes.data_as(C.c_void_p), mesh.name.encode(), 1))
                for mm in fleet:
                    mm._must(mm._L.fp_track_wait(mm.handle, outs.ctypes.data_as(C.c_void_p)))
            tp = timed(submit_all, max(ksteps // K_OBJ, 20), 5)

            def submit_all_host():      # the same from HOST frames: every submission packs its crop window into the model's pinned block
                for mm in fleet:
                    mm._must(mm._L.fp_track_submit(mm.handle, scene.rgb.ctypes.data_as(C.c_void_p), scene.depth.ctypes.data_as(C.c_void_p), 0, H, Wd,
                                                   hyp16.ctypes.data_as(C.c_void_p), mesh.name.encode(), 1))
                for mm in fleet:
                    mm._must(mm._L.fp_track_wait(mm.handle, outs.ctypes.data_as(C.c_void_p)))
            tph = timed(submit_all_host, max(ksteps // K_OBJ, 20), 5)
            pipelined = {"objects_in_flight": K_OBJ, "value": round(K_OBJ * max(ksteps // K_OBJ, 20) / tp, 1), "unit": "tracks/s",
                         "host_frame_value": round(K_OBJ * max(ksteps // K_OBJ, 20) / tph, 1),
                         "what": "one host thread, fp_track_submit for every object then fp_track_wait for every object"}
            for mm in others:
                mm.close()
            # fp_track_multi: the same 8 objects as ONE batch of one model (geometry per object, one refine-net pass over all crops)
            hyps8 = np.tile(hyp16, (K_OBJ, 1)).astype(np.float32)
            outs8 = np.zeros((K_OBJ, 16), np.float32)
            names8 = (C.c_char_p * K_OBJ)(*[mesh.name.encode()] * K_OBJ)

            def multi():
                model._must(model._L.fp_track_multi(model.handle, C.c_void_p(rgb.data_ptr()), C.c_void_p(depth.data_ptr()), 1, H, Wd, K_OBJ,
                                                    hyps8.ctypes.data_as(C.c_void_p), C.cast(names8, C.c_void_p), 1,
                                                    outs8.ctypes.data_as(C.c_void_p)))
            tm = timed(multi, max(ksteps // 4, 50), 5)
            pipelined["batched"] = {"objects": K_OBJ, "ms_per_call": round(tm / max(ksteps // 4, 50) * 1e3, 4),
                                    "value": round(K_OBJ * max(ksteps // 4, 50) / tm, 1), "unit": "tracks/s",
                                    "what": "fp_track_multi: 8 objects of one frame in one batch"}
        extras["track"] = {
            "metric": "Track fps (N=1)", "value": round(ksteps / td, 1), "unit": "frames/s", "ms_per_frame": round(td / ksteps * 1e3, 4),
            "host_frame_value": round(ksteps / thh, 1), "host_frame_ms": round(thh / ksteps * 1e3, 4), "steps": ksteps,
            "pipelined": pipelined,
            "roofline": {"bound": "launch latency (one hipGraph of 21 dependent kernels), not MFMA", "algorithmic_gflop_per_frame": round(tflops / 1e9, 2),
                         "achieved": round(tflops / (td / ksteps) / 1e12, 1), "peak": PEAK_FP16_TFLOPS, "unit": "TFLOP/s",
                         "frac": round(tflops / (td / ksteps) / 1e12 / PEAK_FP16_TFLOPS, 4)},
        }

    # ---- BASELINE configs[3]: 1008 hypotheses (42 views x 24 in-plane steps) sharded exactly like the headline; every rank takes part
    n1008 = None
    if args.full and not args.track and not args.no_extras and args.hyps == 0 and not args.weak:
        model.set_inplane_steps(24)

        k8 = max(3, args.steps // 4)
        t8 = timed(register_dev, k8, 1)
        model.set_inplane_steps(n_total // 42)
        n1008 = {"metric": f"pose-hypotheses/sec (Register N=1008, {Wd}x{H})", "value": round(1008 * k8 / t8, 2), "unit": "hypotheses/s",
                 "ms_per_step": round(t8 / k8 * 1e3, 3), "steps": k8, "n_gpus": world, "scaling": "strong",
                 "workload": f"BASELINE configs[3]: Register N=1008 sharded, {-(-1008 // world)}/GPU, {Wd}x{H}, refine_itr=1, f16"}

    # ---- the other BASELINE configs as short legs of the one --full run (one GPU): configs[4] FP8 1280x720 textured + untextured,
    # configs[1] bf16 Track -- each on its own model / precision, each with its own roofline
    if args.full and not args.no_extras and not args.track and args.dtype == "f16" and (Wd, H) == (640, 480):
        # The 8-bit legs run the DISCRIMINATING synthetic weight set (tests/golden/disc_calib_seed9.npz applied to the seed-9 draws, numpy
        # only): under the headline's plain seed-7 draws the 252 scores agree to 3e-5 and "winner matches" says nothing.  Same
        # architecture, same FLOPs -- the timing does not depend on the weight values.
        disc_cal = W.load_calibration(os.path.join(ROOT, "tests", "golden", "disc_calib_seed9.npz"))
        rp_d, sp_d = os.path.join(wdir, "rd.fpw"), os.path.join(wdir, "sd.fpw")
        W.pack_synthetic("refiner", rp_d, 9, disc_cal)
        W.pack_synthetic("scorer", sp_d, 9, disc_cal)

        def rot_deg(a, b):
            dR = np.einsum("nij,nkj->nik", a[:, :3, :3].astype(np.float64), b[:, :3, :3].astype(np.float64))
            return np.degrees(np.arccos(np.clip((np.trace(dR, axis1=1, axis2=2) - 1) / 2, -1, 1)))

        N_CAL = 16

        def register_leg(textured, dtype, w, h, steps):
            mesh_l = syn.make_mesh(textured=textured)
            # the MEASURED frame is a held-out scene of the synthetic scene family; the calibration sees 16 OTHER frames of it
            scene_l = syn.heldout_scenes(mesh_l, 1, W=w, H=h)[0]
            m = FoundationPose(mesh_l, scene_l.K, rp_d, sp_d, max_input_image_height=max(1080, h), max_input_image_width=max(1920, w))
            try:
                ok, p16, idx16, sc16, ref16, _ = m.register_detailed(scene_l.rgb, scene_l.depth, scene_l.mask, mesh_l.name)
                assert ok, m.last_error
                t_cal = 0.0
                if dtype in Q8:
                    t0 = time.perf_counter()
                    m.calibrate_frames(syn.calibration_scenes(mesh_l, N_CAL, W=w, H=h), mesh_l.name, Q8_PREC[dtype])
                    t_cal = time.perf_counter() - t0
                    m.set_precision(Q8_PREC[dtype])
                ok, p8, idx8, sc8, ref8, _ = m.register_detailed(scene_l.rgb, scene_l.depth, scene_l.mask, mesh_l.name)
                assert ok, m.last_error
                dmm = np.linalg.norm(ref8[:, :3, 3] - ref16[:, :3, 3], axis=1) * 1e3
                ddeg = rot_deg(ref8, ref16)
                # teacher-forced: the f16 networks score the poses the 8-bit refiner produced
                m.set_precision(FP_PREC_F16)
                m.upload_frame(scene_l.rgb, scene_l.depth)
                sc_tf = m.scorer_infer(*m.render_and_transform(mesh_l.name, ref8, 1.1))
                if dtype in Q8:
                    m.set_precision(Q8_PREC[dtype])
                accuracy = {"what": "the f16 path IS the 16-bit reference of this comparison: a second Register of the same model reproduces the first bit for bit",
                            "deterministic": bool(np.array_equal(ref8, ref16) and idx8 == idx16),
                            "parity": "tests/test_precision_gpu.py::test_configs4_f16_720p_follows_the_oracle holds this path to >= 95 % within 1 mm / 1 deg of the fp32 "
                                      "oracle chain (common mode < 0.3 mm) on held-out 1280x720 scenes, textured and untextured"} if dtype not in Q8 else {
                    "weights": "discriminating synthetic set (seed 9 + tests/golden/disc_calib_seed9.npz): score spread ~1, unique maximum",
                    "pose_delta_vs_f16": {"what": "the 252 refined poses against the f16 path's refined pose of the same hypothesis",
                                          "mm_p95": round(float(np.percentile(dmm, 95)), 3), "mm_max": round(float(dmm.max()), 3),
                                          "deg_p95": round(float(np.percentile(ddeg, 95)), 3), "deg_max": round(float(ddeg.max()), 3),
                                          "frac_within_1mm_1deg": round(float(np.mean((dmm < 1) & (ddeg < 1))), 4)},
                    "winner": int(idx8), "winner_f16": int(idx16), "winner_matches_f16": bool(idx8 == idx16),
                    "winner_rank_teacher_forced": int((sc_tf > sc_tf[idx8]).sum()),
                    "score_corr_teacher_forced": round(float(np.corrcoef(sc8, sc_tf)[0, 1]), 4),
                    "winner_pose_delta_vs_f16_winner": {"deg": round(float(rot_deg(p8[None], p16[None])[0]), 3),
                                                        "mm": round(float(np.linalg.norm(p8[:3, 3] - p16[:3, 3]) * 1e3), 3)},
                    "common_mode_mm": round(float(np.linalg.norm((ref8[:, :3, 3] - ref16[:, :3, 3]).mean(0)) * 1e3), 3),
                    "winner_regret_teacher_forced": round(float((sc_tf.max() - sc_tf[idx8]) / (sc_tf.max() - np.median(sc_tf))), 4),
                    "meets_1deg_1mm_for_95pct": bool(np.mean((dmm < 1) & (ddeg < 1)) >= 0.95),
                    "frame": "HELD OUT: a scene the calibration never saw (tests/test_precision_gpu.py measures six such scenes per mesh)",
                }
                r_, d_, k_ = (torch.from_numpy(x).to(dev) for x in (scene_l.rgb, scene_l.depth, scene_l.mask))
                o_ = np.zeros(16, np.float32)

                def fn():
                    m._must(m._L.fp_register_ex(m.handle, C.c_void_p(r_.data_ptr()), C.c_void_p(d_.data_ptr()), C.c_void_p(k_.data_ptr()), 1,
                                                h, w, mesh_l.name.encode(), 1, o_.ctypes.data_as(C.c_void_p)))
                tl = timed(fn, steps, 2)
                m.profile(True)
                m.profile_reset()
                fn()
                pr = m.profile_report()
                m.profile(False)
                roof_l, stages_l, dom_l, _ = analyse_profile(pr, dtype, 252, 2)
                pmc_l = os.path.join(ROOT, "profiles", f"{_Q8_PMC.get(dtype, 'none')}_register_{dtype}_720p_pmc_hbm.json")
                if textured and os.path.exists(pmc_l):
                    for name, rec in json.load(open(pmc_l)).items():
                        if dom_l.split("<")[0].split("[")[0] in name:
                            roof_l["traffic"] = round(rec["traffic_bytes_per_launch"])
                            roof_l["traffic_source"] = os.path.relpath(pmc_l, ROOT)
                            roof_l["traffic_kind"] = "committed rocprofv3 PMC passes of `bench.py --dtype %s --width 1280 --height 720` (profiles/), NOT measured by this run" % dtype
                return {"metric": f"pose-hypotheses/sec (Register N=252, {w}x{h})", "value": round(252 * steps / tl, 2), "unit": "hypotheses/s",
                        "ms_per_step": round(tl / steps * 1e3, 3), "steps": steps, "dtype": dtype,
                        "config": {"workload": f"BASELINE configs[4]: Register N=252 {w}x{h} refine_itr=1, frame resident in HBM, "
                                               f"{'512x512 texture' if textured else '2x2 grey (untextured)'} mesh",
                                   "precision": PRECISION_TEXT[dtype],
                                   "calibration": (f"{N_CAL} held-out frames: fp_calibrate_begin / _add_frame x {N_CAL} / _finish on OTHER scenes of the synthetic scene "
                                                   f"family ({t_cal:.1f} s: per-frame f16 statistics, INT8 weights rounded with error feedback against the frames' "
                                                   "channel means, bias / token / output correction over all frames); the measured frame is not among them") if dtype in Q8 else None},
                        **({"experimental": True, "note": "the 8-bit precisions do NOT hold the configs[4] parity bar (>= 95 % within 1 mm / 1 deg of f16 on every unseen "
                                                          "scene, common mode < 0.3 mm) for any subset of trunk stages (tools/q8_blocks.py, profiles/r06_q8_blocks_*.log; the "
                                                          "bar is a strict xfail in tests/test_precision_gpu.py): configs[4] ships in f16 (legs f16_720p*), this leg is "
                                                          "what the experimental precision costs and reaches"} if dtype in Q8 else
                           {"configs4": "this is the configs[4] path: f16 (DESIGN.md section 4.4: no 8-bit stage subset holds the bar)"}),
                        "accuracy": accuracy, "roofline": roof_l, "stage_ms": dict(list(stages_l.items())[:8])}
            finally:
                m.close()
        lsteps = max(5, args.steps // 2)
        # configs[4] ships in F16 [r6]: legs f16_720p / f16_720p_untextured.  INT8 (calibrated on other frames, measured on a held-out one) is
        # EXPERIMENTAL -- its two legs stay in the line, marked so, with their accuracy objects; FP8 e4m3 is further off: `--fp8-legs` adds its legs
        extras["f16_720p"] = register_leg(True, "f16", 1280, 720, lsteps)
        extras["f16_720p_untextured"] = register_leg(False, "f16", 1280, 720, lsteps)
        extras["int8_720p"] = register_leg(True, "int8", 1280, 720, lsteps)
        extras["int8_720p_untextured"] = register_leg(False, "int8", 1280, 720, lsteps)
        if args.fp8_legs:
            extras["fp8_720p"] = register_leg(True, "fp8", 1280, 720, lsteps)
            extras["fp8_720p_untextured"] = register_leg(False, "fp8", 1280, 720, lsteps)
        # Track in INT8 (discriminating weights, calibrated on the bench frame): the 8-bit weights halve the per-layer weight stream that
        # bounds a conv at N = 1
        def track_leg_int8(steps):
            mesh_l = syn.make_mesh()
            scene_l = syn.make_scene(mesh_l, Wd, H)
            m = FoundationPose(mesh_l, scene_l.K, rp_d, sp_d)
            try:
                m.calibrate_frames(syn.calibration_scenes(mesh_l, N_CAL, W=Wd, H=H), mesh_l.name, FP_PREC_INT8)   # (the tracked frame is not among them)
                r_, d_ = (torch.from_numpy(x).to(dev) for x in (scene_l.rgb, scene_l.depth))
                hyp_l = syn.to_colmajor(syn.perturb_pose(scene_l.gt_pose))
                o_ = np.zeros(16, np.float32)

                def fn():
                    m._must(m._L.fp_track_ex(m.handle, C.c_void_p(r_.data_ptr()), C.c_void_p(d_.data_ptr()), 1, H, Wd,
                                             hyp_l.ctypes.data_as(C.c_void_p), mesh_l.name.encode(), 1, o_.ctypes.data_as(C.c_void_p)))
                m.set_precision(FP_PREC_F16)
                fn()
                p16 = o_.reshape(4, 4).T.copy()
                m.set_precision(FP_PREC_INT8)
                fn()
                p8 = o_.reshape(4, 4).T.copy()
                tl = timed(fn, steps, 10)
                return {"metric": "Track fps (N=1)", "value": round(steps / tl, 1), "unit": "frames/s", "ms_per_frame": round(tl / steps * 1e3, 4), "steps": steps,
                        "dtype": "int8", "config": {"workload": f"Track N=1 {Wd}x{H}, INT8 trunk convolutions (calibrated on 16 OTHER frames), frame resident in HBM",
                                                    "weights": "discriminating synthetic set"},
                        "accuracy": {"pose_delta_vs_f16_track": {"deg": round(float(rot_deg(p8[None], p16[None])[0]), 3),
                                                                 "mm": round(float(np.linalg.norm(p8[:3, 3] - p16[:3, 3]) * 1e3), 3)}},
                        "graph": "21 kernels (row ranges inside the vertex + crop launch, the encoder tail of both heads in one launch); the f16 graph spans 192.5 us (profiles/r05d_track_timeline.txt)"}
            finally:
                m.close()
        extras["track_int8"] = track_leg_int8(max(args.steps * 10, 100))
        # configs[1]: Track, N = 1, bf16 refine-net
        model.set_precision(FP_PREC_BF16)
        kb = max(args.steps * 5, 50)
        tb = timed(track_dev, kb, 10)
        model.profile(True)
        model.profile_reset()
        track_dev()
        bprof = model.profile_report()
        model.profile(False)
        model.set_precision(0)
        bflops = sum(v["flops"] for k, v in bprof.items() if k.startswith("conv_") or k.startswith("gemm_") or k == "attention")
        extras["track_bf16"] = {
            "metric": "Track fps (N=1)", "value": round(kb / tb, 1), "unit": "frames/s", "ms_per_frame": round(tb / kb * 1e3, 4), "steps": kb,
            "dtype": "bf16", "config": {"workload": f"BASELINE configs[1]: Track N=1 {Wd}x{H}, bf16 refine-net, frame resident in HBM"},
            "roofline": {"bound": "launch latency (one hipGraph of dependent kernels), not MFMA", "algorithmic_gflop_per_frame": round(bflops / 1e9, 2),
                         "achieved": round(bflops / (tb / kb) / 1e12, 1), "peak": PEAK_FP16_TFLOPS, "unit": "TFLOP/s",
                         "frac": round(bflops / (tb / kb) / 1e12 / PEAK_FP16_TFLOPS, 4), "launches_in_eager_profile": sum(v["calls"] for v in bprof.values()), "graph_kernels": 21, "note": "the profiled call runs eagerly with pose update and heads as separate launches; the replayed graph has 21 kernels (profiles/r05d_track_timeline.txt)"}}
    if n1008 is not None:
        extras["n1008"] = n1008

    units = 1 if args.track else n_total
    ms = dt / args.steps * 1e3
    roofline, stages = None, None
    if args.full:
        roof, stages, dom, dv = analyse_profile(prof, args.dtype, n_total // world if world > 1 else n_total, 1 if args.track else 2)
        traffic, traffic_src = None, None
        pmc_path = os.path.join(ROOT, "profiles", PMC_FILE)
        if args.dtype in Q8 and (Wd, H) == (1280, 720):
            pmc_path = os.path.join(ROOT, "profiles", f"{_Q8_PMC[args.dtype]}_register_{args.dtype}_720p_pmc_hbm.json")
        if os.path.exists(pmc_path) and not args.track and world == 1 and ((args.dtype == "f16" and (Wd, H) == (640, 480)) or (args.dtype in Q8 and (Wd, H) == (1280, 720))):
            pmc = json.load(open(pmc_path))
            for name, rec in pmc.items():
                if dom.split("<")[0].split("[")[0] in name:
                    traffic, traffic_src = round(rec["traffic_bytes_per_launch"]), os.path.relpath(pmc_path, ROOT)
        # the same fraction recomputed from the committed rocprofv3 kernel-stats summary (its average duration of the dominant kernel x this
        # run's algorithmic FLOPs per launch): the HIP-event figure above and the profiler's must agree
        recomputed = None
        stats_path = os.path.join(ROOT, "profiles", STATS_FILE)
        if os.path.exists(stats_path) and not args.track and args.dtype == "f16" and (Wd, H) == (640, 480) and n_total == 252:
            import csv
            key = dom.split("<")[0].split("[")[0]
            rows = [r for r in csv.DictReader(open(stats_path)) if key in r["Name"]]
            if rows:
                top = max(rows, key=lambda r: float(r["TotalDurationNs"]))
                avg_ms = float(top["AverageNs"]) * 1e-6
                ach = roof["algorithmic_gflop_per_launch"] / avg_ms      # GFLOP / ms = TFLOP/s
                recomputed = {"source": os.path.relpath(stats_path, ROOT), "kernel": top["Name"], "calls": int(top["Calls"]), "avg_launch_ms": round(avg_ms, 4),
                              "achieved": round(ach, 1), "frac": round(ach / roof["peak"], 4),
                              "what": "rocprofv3 --kernel-trace --stats average of the dominant kernel (a committed run on another box of the pool) x this run's algorithmic GFLOP per launch"}
        # what the matrix pipes sustain on THIS box with every SIMD busy (register-resident MFMAs, random operands): the
        # datasheet 2.5 PFLOP/s assumes 2.4 GHz, under MFMA load the power limit holds the clock near 2.0 GHz
        measured_peak, measured_mhz, peak_detail = None, None, None
        if world == 1 and not args.no_mfma_peak:
            from foundationpose_cpp_amd import _lib
            L = _lib.test_lib()   # the micro-benchmark kernel lives in the test build
            L.fpt_mfma_peak.restype = C.c_float
            L.fpt_mfma_peak.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
            mhz = C.c_double(0)
            v = max(L.fpt_mfma_peak(200000, 8, 0, C.byref(mhz)) for _ in range(2))
            if v > 0:
                measured_peak, measured_mhz = round(float(v), 1), round(mhz.value)
            # the evidence behind "power-limited": both MFMA shapes with random and with all-zero operands (zero operands toggle no
            # data-path bits: same instruction stream, less power, higher clock), and the package power / clocks rocm-smi reports
            # WHILE the random-operand kernel runs (sampled from this thread, the kernel loops on another)
            peak_detail = {}
            for tag, code in (("16x16x32_random", 0), ("16x16x32_zero", 1), ("32x32x16_random", 2), ("32x32x16_zero", 3)):
                m2 = C.c_double(0)
                v2 = max(L.fpt_mfma_peak(200000, 8, code, C.byref(m2)) for _ in range(2))
                peak_detail[tag] = {"tflops": round(float(v2), 1), "shader_clock_mhz": round(m2.value)}
            try:
                import subprocess, threading
                stop = threading.Event()

                def burn():
                    while not stop.is_set():
                        L.fpt_mfma_peak(400000, 8, 0, None)
                th = threading.Thread(target=burn)
                th.start()
                time.sleep(0.4)
                smi = subprocess.run(["rocm-smi", "--showpower", "--showclocks", "--showmaxpower", "--json"], capture_output=True, text=True, timeout=20)
                stop.set()
                th.join()
                card = next(iter(json.loads(smi.stdout).values()))
                keep = {k: v for k, v in card.items() if any(t in k.lower() for t in ("power", "sclk", "mclk", "fclk"))}
                peak_detail["rocm_smi_under_mfma_load"] = keep
            except Exception as e:     # (no rocm-smi on the box / unexpected output: the clocks above are the evidence)
                peak_detail["rocm_smi_under_mfma_load"] = {"error": str(e)[:200]}
        # where the dominant kernel's other half goes: in-kernel clock probe of conv_halo_kernel on the conv_256 shape (test build,
        # outside every timed region): shader clock the package allows under this load, cycles of a workgroup's main loop, and the
        # share of them in which its SIMD's matrix pipe is issuing (2 co-resident waves x 72 K-steps x 40 MFMAs x 16 cycles)
        clock_probe = None
        if world == 1 and not args.no_mfma_peak and not args.track and args.dtype == "f16":
            try:
                from foundationpose_cpp_amd import _lib
                Lt = _lib.test_lib()
                rng = np.random.default_rng(0)
                NBp = 126
                xp = rng.standard_normal((NBp, 40, 40, 256), dtype=np.float32)
                wp = (rng.standard_normal((256, 3, 3, 256), dtype=np.float32) / 48.0).astype(np.float32)
                bp = np.zeros(256, np.float32)
                op = np.zeros((NBp, 40, 40, 256), np.float32)
                msf = C.c_float(0)
                pp_ = lambda t: t.ctypes.data_as(C.c_void_p)  # noqa: E731
                if Lt.fpt_clk_probe(1 << 16, None, None) == 0 and \
                        Lt.fpt_conv(pp_(xp), pp_(wp), pp_(bp), None, NBp, 40, 40, 256, 256, 3, 3, 1, 1, 40, 40, 1, 0, pp_(op), 3, C.byref(msf)) == 0:
                    mhz_p, cyc_p = C.c_double(0), C.c_double(0)
                    Lt.fpt_clk_probe(-512, C.byref(mhz_p), C.byref(cyc_p))
                    if cyc_p.value > 0:
                        issue = 2 * 72 * 40 * 16 / cyc_p.value
                        clock_probe = {"kernel": "conv_halo_kernel (conv_256 shape, 126 hypotheses)", "shader_clock_mhz": round(mhz_p.value),
                                       "main_loop_cycles_per_workgroup": round(cyc_p.value),
                                       "mfma_issue_share_of_main_loop": round(issue, 3),
                                       "clock_vs_datasheet_2400": round(mhz_p.value / 2400.0, 3),
                                       "what": "0.5 of the datasheet peak = issue share in the loop x loop share of a round (~0.84) x round fill x "
                                               "clock / 2.4 GHz: the package's power limit, not the schedule, is the largest factor (DESIGN.md section 8)"}
            except Exception as e:   # evidence only: never fail the bench over it
                clock_probe = {"error": str(e)}
        roofline = dict(roof, **{
            "peak_measured": measured_peak, "peak_measured_clock_mhz": measured_mhz, "peak_measured_detail": peak_detail,
            "peak_measured_what": "register-resident f16 MFMA micro-benchmark on this box (fp8 MFMAs: 2x)",
            "frac_of_measured": round(roof["achieved"] / (measured_peak * (2 if dv.get("fp8") else 1)), 4) if measured_peak else None,
            "clock_probe": clock_probe,
            "recomputed_from_profiles": recomputed,
            "traffic": traffic, "traffic_source": traffic_src,
            "traffic_kind": "committed rocprofv3 PMC passes of the same command (profiles/), NOT measured by this run" if traffic else None,
        })
    res = {
        "metric": "Track fps (N=1)" if args.track else f"pose-hypotheses/sec (Register N={n_total}, {Wd}x{H})",
        "value": round(units * args.steps / dt, 2),
        "unit": "frames/s" if args.track else "hypotheses/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3),
        "higher_is_better": True,
        "scaling": "weak" if args.weak and args.hyps == 0 else "strong",
        # the reference's number is timed around the host-frame call (speed_register): compare like with like when that leg ran
        "vs_baseline": None if args.track else round((extras["host_frame"]["value"] if "host_frame" in extras and n_total == 252
                                                      else units * args.steps / dt) / BASELINE_HYP_S, 3),
        "dtype": args.dtype, "data": "synthetic",
        "config": {
            "workload": (f"Track N=1 {Wd}x{H}" if args.track else
                         f"Register N={n_total} hypotheses" + (f" sharded, {-(-n_total // world)}/GPU," if world > 1 else ",") +
                         f" {Wd}x{H} refine_itr=1, frame resident in HBM"),
            "mesh": f"synthetic ellipsoid V=2562 F=5120, {'2x2 grey (untextured)' if args.untextured else '512x512 texture'}",
            "weights": "synthetic (seed 7)",
            "precision": PRECISION_TEXT[args.dtype],
            "calibration": "16 frames of OTHER synthetic scenes (fp_calibrate_begin / _add_frame / _finish); the bench frame is not among them" if args.dtype in Q8 else None,
            "parallelism": f"hyp-shard x{world}" if world > 1 else "single GPU",
            "collective": "none",
            "baseline": "reference README.md:37-41 Register 2.8 fps x 252 = 705.6 hyp/s on RTX 4060 (TensorRT fp16), timed around the host-frame "
                        "call; vs_baseline = host_frame.value / 705.6 when that leg ran (N=1 --full run), else value / 705.6",
        },
    }
    if roofline is not None:
        res["roofline"] = roofline
        res["stage_ms"] = stages
    res.update(extras)
    if args.full and not args.no_cpu_baseline and world == 1:
        res["cpu_baseline"] = cpu_baseline(mesh, scene, states)
    model.close()
    # RCCL prints a version banner through C stdio (flushed only at exit when stdout is a pipe): every rank pushes its buffered
    # output out, THEN rank 0 prints, so that the JSON line is the last line of the job's stdout
    sys.stdout.flush()
    try:
        C.CDLL(None).fflush(None)
    except OSError:
        pass
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
