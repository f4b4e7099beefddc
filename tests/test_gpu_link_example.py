"""examples/sage_link_call_groups.py learns: link prediction over ``LinkNeighborLoader.call_groups()`` with the one-kernel
head (``nn.link_bce_with_logits``) tells the planted partition's edges from random pairs, and as well as the same loop with the
torch-op head does."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sage_link_call_groups_example_learns_like_the_torch_op_head(hiplib):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import sage_link_call_groups as ex
    argv = ["--nodes", "4000", "--epochs", "2", "--batch-size", "128", "--group", "4"]      # 24 optimizer steps per epoch
    loss, acc = ex.main(argv)
    loss_t, acc_t = ex.main(argv + ["--torch-ops"])
    what = "kernel head: loss %.4f accuracy %.4f; torch-op head: loss %.4f accuracy %.4f" % (loss, acc, loss_t, acc_t)
    print(what)
    # chance is 0.5 (as many negatives as positives); an epoch scores 24 000 pairs, so 0.52 is six standard errors above it
    assert acc > 0.52, what
    assert abs(acc - acc_t) <= 0.02, what
