"""examples/temporal_hetero_link_call_groups.py runs both of its loops — temporal ``hetero_call_groups()`` with one optimizer step
per group, and ``--per-batch`` — over the same epoch: the same pairs and, sampling being independent of the model, the same
number of temporal edges sampled by the call-group walk as by the one-batch-at-a-time route."""
import math
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("fanout", [["5", "5"], ["3", "2", "2"]], ids=["2-hops", "3-hops"])
def test_temporal_hetero_link_example_runs_both_loops_over_the_same_samples(hiplib, fanout):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import temporal_hetero_link_call_groups as ex
    # 1000 seed edges: 7 full batches of 128 in groups of 4, and a ragged batch of 104; 2 negatives per positive
    argv = ["--users", "1500", "--items", "400", "--avg-degree", "10", "--epochs", "1", "--batch-size", "128", "--group", "4",
            "--train-edges", "1000", "--fanout"] + fanout
    loss, acc = ex.main(argv)
    groups = dict(ex.LAST_EPOCH)
    loss_b, acc_b = ex.main(argv + ["--per-batch"])
    batches = dict(ex.LAST_EPOCH)
    print("call groups: loss %.4f accuracy %.3f, %d edges; per batch: loss %.4f accuracy %.3f, %d edges"
          % (loss, acc, groups["sampled_edges"], loss_b, acc_b, batches["sampled_edges"]))
    assert groups["pairs"] == batches["pairs"] == 3 * 1000
    assert groups["sampled_edges"] == batches["sampled_edges"] > 0
    assert math.isfinite(loss) and math.isfinite(loss_b) and 0.0 <= acc <= 1.0 and 0.0 <= acc_b <= 1.0
