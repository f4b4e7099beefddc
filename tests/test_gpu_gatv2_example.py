"""examples/gatv2_call_group_training.py learns: two GATv2Conv layers (features -> 4 x 64 concatenated -> classes, one head
averaged) over ``NeighborLoader.call_groups()`` find the planted communities, on the attention kernels.

The accuracy yardstick is the same model in float64 torch ops on the same synthetic data, which the example runs itself on the
CPU (mini-batches sampled by its torch restatement of the loader):
    python examples/gatv2_call_group_training.py --nodes 30000 --epochs 6 --batch-size 256 --group 4 --fanout 10 5 \
        --torch-ops --float64 --device cpu
reaches a training accuracy of 0.954 in its last epoch (loss 2.0205 -> 0.1734).  The example on the HIP kernels has to come
within 5 points of that — the margin test_gpu_gin_example.py grants float32 trajectories, here also over other samples — and
its loss has to fall and end below ln(classes)."""
import json
import math
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT64_TORCH_OPS_ACCURACY = 0.954
CLASSES = 16


def test_gatv2_call_group_example_learns(hiplib):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "gatv2_call_group_training.py"), "--nodes", "30000", "--epochs", "6",
           "--batch-size", "256", "--group", "4", "--fanout", "10", "5"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    print(res.stdout)
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["route"] == "kernel", out
    assert out["last_loss"] < out["first_loss"] and out["last_loss"] < math.log(CLASSES), out
    assert out["accuracy"] >= FLOAT64_TORCH_OPS_ACCURACY - 0.05, out
