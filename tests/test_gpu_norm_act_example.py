"""examples/mag_encoder_call_groups.py at a tiny size: the reference's encoder (conv + lin1 residual, LayerNorm, Dropout(0.5),
ReLU, twice, then lin2 -> relu) trains on either route of the block between the layers."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("torch_ops", [False, True])
def test_mag_encoder_example_learns(hiplib, monkeypatch, torch_ops):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import mag_encoder_call_groups as ex
    monkeypatch.setattr(sys, "argv", ["x", "--items", "4000", "--epochs", "2", "--batch-size", "128", "--group", "2"]
                        + (["--torch-ops"] if torch_ops else []))
    res = ex.main()
    assert (res["block_launches"] > 0) != torch_ops               # the fused block launches, the torch chain never does
    assert (res["other"]["block_launches"] > 0) == torch_ops      # and the other route ran too, for its times
    assert len(res["epoch_ms"]) == len(res["other"]["epoch_ms"]) == 2
    losses, q = res["losses"], max(len(res["losses"]) // 4, 1)
    assert sum(losses[-q:]) / q < sum(losses[:q]) / q, losses     # the loss falls
    assert res["accuracy"] > 0.18, res["accuracy"]                 # chance: 1 / 8 (five sigma of 1024 held-out items above it)
    assert res["eval_repeatable"], "two eval passes agree exactly"
