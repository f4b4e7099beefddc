"""examples/rgcn_call_group_training.py learns: the RGCN call-group loop (trainable emb[n_id] input, relation ids through
CallGroup.edge_attr, one-kernel RGCN layers forward and backward, one optimizer step per call group) reads the labels
through the relation-typed neighbours."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rgcn_call_group_training_example_learns(hiplib, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import rgcn_call_group_training as ex
    monkeypatch.setattr(sys, "argv", ["x", "--nodes", "20000", "--epochs", "4", "--batch-size", "256", "--group", "4"])
    loss, acc = ex.main()
    assert loss < 1.0 and acc > 0.7, (loss, acc)    # chance: ln 8 = 2.08, 1 / 8
