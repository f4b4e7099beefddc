"""examples/row_linear_projection.py at a tiny size, a fresh child process per route: the skeleton of the reference's Classifier
(projection with LayerNorm over a bfloat16 table, two SAGE layers, relu -> normalize -> add tail, linear head) trains through
``nn.RowLinear`` as it does through torch.nn.functional, from the same seed."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def runs(hiplib):
    out = {}
    for torch_ops in (False, True):
        cmd = [sys.executable, os.path.join(ROOT, "examples", "row_linear_projection.py"), "--nodes", "3000", "--epochs", "3",
               "--batch-size", "128", "--group", "2", "--json"] + (["--torch-ops"] if torch_ops else [])
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        out[torch_ops] = json.loads(p.stdout.strip().splitlines()[-1])
    return out


@pytest.mark.gpu
def test_both_routes_train_from_the_same_start(runs):
    kernel, torch_ops = runs[False], runs[True]
    assert kernel["routes"] == ["kernel", "kernel", "kernel"] and kernel["row_linear_launches"] == 3 * len(kernel["losses"])
    assert torch_ops["row_linear_launches"] == 0
    assert len(kernel["losses"]) == len(torch_ops["losses"]) >= 12
    a, b = kernel["losses"][0], torch_ops["losses"][0]
    assert abs(a - b) <= 1e-5 * abs(b), (a, b)
    for res in (kernel, torch_ops):
        losses, q = res["losses"], max(len(res["losses"]) // 4, 1)
        assert sum(losses[-q:]) / q < sum(losses[:q]) / q, losses     # the loss falls
