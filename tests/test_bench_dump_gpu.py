"""bench.py --dump-outputs: the arrays written after the timed steps are what the headline's last timed step handed its caller, on the
seeded inputs every run of bench.py uses, and --steps is the number of timed steps the JSON line reports."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
QUICK = ["--no-extras", "--no-cpu-baseline", "--no-mfma-peak"]


def _bench(out_dir, **env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "FP_RDV_ADDR", "FP_BENCH_STUB_RANK", "FP_BENCH_FORCE_SHARD")}
    env.update(env_extra)
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir)] + QUICK,
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["steps"] == 3 and res["warmup"] == 1
    out = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir)}
    pose = out["pose"]
    assert pose.dtype == np.float32 and pose.shape == (4, 4) and np.isfinite(pose).all()
    return out


def _weights(tmp_path):
    from foundationpose_cpp_amd import weights as W
    rp, sp = str(tmp_path / "r.fpw"), str(tmp_path / "s.fpw")
    W.pack_synthetic("refiner", rp)
    W.pack_synthetic("scorer", sp)
    return rp, sp


@pytest.mark.gpu
def test_dump_outputs_is_the_register_pose(tmp_path, syn_mesh, syn_scene):
    from foundationpose_cpp_amd import FoundationPose
    out = _bench(tmp_path / "out")
    assert sorted(out) == ["pose"]
    m = FoundationPose(syn_mesh, syn_scene.K, *_weights(tmp_path), max_input_image_height=1080, max_input_image_width=1920)
    ok, ref = m.Register(syn_scene.rgb, syn_scene.depth, syn_scene.mask, syn_mesh.name)
    m.close()
    assert ok
    np.testing.assert_allclose(out["pose"], ref, rtol=0, atol=1e-6)


@pytest.mark.gpu
def test_dump_outputs_of_the_sharded_path(tmp_path, syn_mesh, syn_scene):
    """the one-rank run of the sharded body (fp_register_sharded): the pose is the refined pose of the winner it reports"""
    from foundationpose_cpp_amd import FoundationPose
    out = _bench(tmp_path / "out", FP_BENCH_FORCE_SHARD="1")
    assert sorted(out) == ["pose", "winner"]
    assert out["winner"].dtype == np.float64 and out["winner"].shape == (1,)
    idx = int(out["winner"][0])
    assert idx == out["winner"][0] and 0 <= idx < 252
    m = FoundationPose(syn_mesh, syn_scene.K, *_weights(tmp_path), max_input_image_height=1080, max_input_image_width=1920)
    ok, _, _, _, refined, _ = m.register_detailed(syn_scene.rgb, syn_scene.depth, syn_scene.mask, syn_mesh.name)
    m.close()
    assert ok
    pose, ref = out["pose"], refined[idx]
    ddeg = np.degrees(np.arccos(np.clip((np.trace(pose[:3, :3] @ ref[:3, :3].T) - 1) / 2, -1, 1)))
    assert np.linalg.norm(pose[:3, 3] - ref[:3, 3]) < 1e-4 and ddeg < 0.1     # tests/sharded_native_worker.py's bar
