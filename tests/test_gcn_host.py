"""Host-side checks of wholegraph_amd.nn.GCNConv (no GPU): PyG's parameter names, shapes and initialisation, the refusal of
``cached=True``, and the float64 gcn_norm restatement the GPU tests measure against (tests/gcn_ref.py) against A_hat
computed by hand."""
import math

import pytest
import torch

from gcn_ref import dense_a_hat


def test_parameters_match_pyg():
    from wholegraph_amd.nn import GCNConv
    torch.manual_seed(0)
    conv = GCNConv(100, 256)
    sd = conv.state_dict()
    assert sorted(sd.keys()) == ["bias", "lin.weight"]
    assert sd["lin.weight"].shape == (256, 100) and sd["bias"].shape == (256,)
    assert bool((sd["bias"] == 0).all())
    bound = math.sqrt(6.0 / (100 + 256))       # glorot
    w = sd["lin.weight"]
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound
    assert abs(float(w.std()) - bound / math.sqrt(3)) < 0.05 * bound
    assert conv.lin.bias is None
    # a state dict shaped like PyG's loads unchanged
    want = {"lin.weight": torch.randn(256, 100), "bias": torch.randn(256)}
    conv.load_state_dict(want)
    assert torch.equal(conv.lin.weight.detach(), want["lin.weight"]) and torch.equal(conv.bias.detach(), want["bias"])
    assert GCNConv(8, 4, bias=False).bias is None
    assert set(GCNConv(8, 4, bias=False).state_dict()) == {"lin.weight"}


def test_cached_is_refused():
    from wholegraph_amd.nn import GCNConv
    with pytest.raises(ValueError, match="cached"):
        GCNConv(4, 4, cached=True)


def _ei(pairs):
    return torch.tensor(pairs, dtype=torch.long).t()      # [(src, dst), ...] -> [2, E]


def _check(got, want):
    assert torch.allclose(got, torch.tensor(want, dtype=torch.float64), atol=1e-14), got


def test_gcn_norm_isolated_node_and_plain_edges():
    # 0 -> 1, 2 -> 1; node 3 isolated.  deg (with loops): 1, 3, 1, 1
    a = dense_a_hat(_ei([(0, 1), (2, 1)]), 4)
    s3 = 1 / math.sqrt(3)
    _check(a, [[1, 0, 0, 0], [s3, 1 / 3, s3, 0], [0, 0, 1, 0], [0, 0, 0, 1]])


def test_gcn_norm_existing_self_loop_and_duplicate_edge():
    # 0 -> 1 twice (counted twice), 1 -> 1 with weight 3 (becomes the loop, not counted again), 1 -> 0
    ei = _ei([(0, 1), (0, 1), (1, 1), (1, 0)])
    a = dense_a_hat(ei, 2, edge_weight=torch.tensor([1.0, 1.0, 3.0, 1.0]))
    d0, d1 = 2.0, 5.0           # node 0: loop 1 + edge from 1; node 1: loop 3 + two copies of 0 -> 1
    _check(a, [[1 / d0, 1 / math.sqrt(d0 * d1)], [2 / math.sqrt(d0 * d1), 3 / d1]])
    # unweighted: the existing loop keeps weight 1 even when improved (fill only for nodes without one)
    a = dense_a_hat(_ei([(1, 1), (0, 1)]), 2, improved=True)
    d0, d1 = 2.0, 2.0
    _check(a, [[2 / d0, 0], [1 / math.sqrt(d0 * d1), 1 / d1]])


def test_gcn_norm_improved():
    a = dense_a_hat(_ei([(0, 1)]), 2, improved=True)
    d0, d1 = 2.0, 3.0
    _check(a, [[2 / d0, 0], [1 / math.sqrt(d0 * d1), 2 / d1]])


def test_gcn_norm_without_self_loops():
    # node 0 has in-degree 0: factor 0 (inf -> 0); the loop edge 1 -> 1 is an ordinary edge
    a = dense_a_hat(_ei([(0, 1), (1, 1), (1, 2)]), 3, add_self_loops=False)
    d = [0.0, 2.0, 1.0]
    inv = [0.0 if v == 0 else 1 / math.sqrt(v) for v in d]
    _check(a, [[0, 0, 0], [inv[1] * inv[0], inv[1] * inv[1], 0], [0, inv[2] * inv[1], 0]])


def test_gcn_norm_unnormalized():
    a = dense_a_hat(_ei([(0, 1), (0, 1), (1, 1)]), 2, edge_weight=torch.tensor([0.5, 2.0, 3.0]), normalize=False)
    _check(a, [[0, 0], [2.5, 3.0]])
