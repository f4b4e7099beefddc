"""examples/transformer_link_prediction.py learns: mag_lp_mnmg.py's encoder (two TransformerConv(edge_dim=1) layers with a
per-edge attribute read through batch.e_id, LayerNorm, L2 normalisation, dot-product decoder) over LinkNeighborLoader
batches with binary negatives separates the planted intra-community edges from random pairs well above chance."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_transformer_link_prediction_example_learns(hiplib, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import transformer_link_prediction as ex
    monkeypatch.setattr(sys, "argv", ["x", "--nodes", "8000", "--epochs", "3", "--batch-size", "256"])
    loss, acc = ex.main()
    assert loss < 0.6 and acc > 0.75, (loss, acc)     # chance: ln 2 = 0.69, 1 / 2
