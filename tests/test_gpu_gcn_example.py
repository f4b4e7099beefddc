"""examples/gcn_call_group_training.py learns: the GCN call-group loop (lazy features, one-kernel GCN layers forward and
backward, one optimizer step per call group) recovers the planted communities."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gcn_call_group_training_example_learns(hiplib, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import gcn_call_group_training as ex
    monkeypatch.setattr(sys, "argv", ["x", "--nodes", "30000", "--epochs", "6", "--batch-size", "256", "--group", "4",
                                      "--fanout", "10", "5"])
    loss, acc = ex.main()
    assert loss < 1.5 and acc > 0.6, (loss, acc)
