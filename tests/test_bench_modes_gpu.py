"""bench.py --gpus 1: a plain run prints the headline and nothing that needs runs of its own; --full adds them after the same timed
steps (here the per-kernel profile step behind `roofline` and `stage_ms`, with the slower legs switched off)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup"}
FULL_ONLY = {"roofline", "stage_ms", "cpu_baseline", "host_frame", "track", "track_bf16", "track_int8", "n1008",
             "f16_720p", "f16_720p_untextured", "int8_720p", "int8_720p_untextured"}


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "FP_RDV_ADDR", "FP_BENCH_STUB_RANK", "FP_BENCH_FORCE_SHARD")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", *extra],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert HEADLINE <= set(res), sorted(HEADLINE - set(res))
    assert res["metric"] == "pose-hypotheses/sec (Register N=252, 640x480)" and res["unit"] == "hypotheses/s"
    assert res["higher_is_better"] is True and res["dtype"] == "f16" and res["n_gpus"] == 1
    assert res["steps"] == 3 and res["warmup"] == 1
    assert abs(res["value"] - 252e3 / res["ms_per_step"]) <= 1e-3 * res["value"]
    return res


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone():
    res = _bench()
    assert not FULL_ONLY & set(res), sorted(FULL_ONLY & set(res))


@pytest.mark.gpu
def test_full_run_adds_the_profile_and_roofline():
    res = _bench("--full", "--no-extras", "--no-cpu-baseline", "--no-mfma-peak")
    assert res["roofline"]["kernel"] != "none" and res["roofline"]["achieved"] > 0
    assert res["stage_ms"] and all(v >= 0 for v in res["stage_ms"].values())
    assert not {"cpu_baseline", "host_frame", "track", "n1008"} & set(res)
