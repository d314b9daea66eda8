"""bench.py on one GPU: a plain run times the headline and nothing else; `--full` adds the sub-records and the CPU leg."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")
FULL_ONLY = ("cpu_baseline", "parity", "variant_block_bfgs_ms", "small_batches_ms", "gpu_over_cpu_all_cores", "qp_replay", "configs", "reference_tests")


def _bench(tmp_path, *extra):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    detail = tmp_path / "detail.json"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "512",
                          "--detail-out", str(detail), *extra], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    allout = [l for l in out.stdout.splitlines() if l.strip()]
    lines = [l for l in allout if l.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) < 4096 and allout[-1] == lines[0], allout
    line = json.loads(lines[0])
    for k in CONTRACT_KEYS:
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["dtype"] == "f64" and line["higher_is_better"] is True
    assert line["value"] > 0 and line["ms_per_step"] > 0
    return line, json.load(open(detail))


@pytest.mark.gpu
def test_plain_run_times_the_headline_only(tmp_path):
    line, detail = _bench(tmp_path)
    assert not [k for k in FULL_ONLY if k in line], line
    assert not [k for k in ("cpu_baseline", "parity_vs_cpu_same_order", "parity_vs_cpu_reference", "variant_block_bfgs", "small_batches", "configs",
                            "reference_tests", "qp_replay") if k in detail], sorted(detail)


@pytest.mark.gpu
def test_full_run_adds_the_sub_records_and_the_cpu_leg(tmp_path):
    line, detail = _bench(tmp_path, "--full", "--configs", "", "--no-replay", "--cpu-sample", "64", "--cpu-seconds", "0.2")
    for k in ("cpu_baseline", "parity", "variant_block_bfgs_ms", "small_batches_ms", "gpu_over_cpu_all_cores"):
        assert k in line, k
    assert sorted(line["small_batches_ms"]) == ["1", "512", "64"]
    assert line["parity"]["same_order_bit_identical"] is True
    assert detail["parity_vs_cpu_same_order"]["instances"] == 64 and detail["cpu_baseline"]["value"] > 0
