"""examples/hetero_link_call_groups.py learns: heterogeneous link prediction over ``LinkNeighborLoader.hetero_call_groups()`` —
typed ``user -> item`` seed edges, two ``HeteroConv`` of ``SAGEConv`` layers, the one-kernel head of either decoder — tells the
planted bipartite graph's edges from random pairs, and as well as the same loop with the torch-op head does."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 4000 users x 12 `rates` edges, a quarter of them seed edges: 12 000 positives + 12 000 negatives
N_PAIRS = 24_000


@pytest.mark.parametrize("decoder", ["mlp", "dot"])
def test_hetero_link_call_groups_example_learns_like_the_torch_op_head(hiplib, decoder):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import hetero_link_call_groups as ex
    argv = ["--users", "4000", "--items", "3000", "--epochs", "2", "--batch-size", "128", "--group", "4", "--decoder", decoder]
    loss, acc = ex.main(argv)                    # 24 optimizer steps per epoch
    assert ex.LAST_EPOCH["pairs"] == N_PAIRS
    loss_t, acc_t = ex.main(argv + ["--torch-ops"])
    what = "%s, kernel head: loss %.4f accuracy %.4f; torch-op head: loss %.4f accuracy %.4f" % (decoder, loss, acc, loss_t, acc_t)
    print(what)
    # chance is 0.5 (as many negatives as positives); an epoch scores N = 24 000 pairs: six standard errors above chance
    assert acc > 0.5 + 6 * 0.5 / N_PAIRS ** 0.5, what
    assert abs(acc - acc_t) <= 0.02, what
