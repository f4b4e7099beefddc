"""Host-side checks of wholegraph_amd.nn.RGCNConv (no GPU): PyG's parameter names, shapes and initialisation, the refusals
(num_blocks, aggr="max", featureless input), FastRGCNConv as the same class, and the float64 restatement the GPU tests measure
against (tests/rgcn_ref.py) against a dense per-relation adjacency built by hand."""
import math

import pytest
import torch

from rgcn_ref import dense_relation_adjacency, relation_weights, rgcn_forward


def _glorot_ok(p):
    bound = math.sqrt(6.0 / (p.size(-2) + p.size(-1)))
    m = float(p.detach().abs().max())
    assert 0.8 * bound < m <= bound, (m, bound)


@pytest.mark.parametrize("kw,keys", [
    ({"num_bases": 30}, {"weight": (30, 32, 16), "comp": (535, 30), "root": (32, 16), "bias": (16,)}),
    ({}, {"weight": (535, 32, 16), "root": (32, 16), "bias": (16,)}),
    ({"root_weight": False}, {"weight": (535, 32, 16), "bias": (16,)}),
    ({"bias": False, "num_bases": 4}, {"weight": (4, 32, 16), "comp": (535, 4), "root": (32, 16)}),
])
def test_parameters_match_pyg(kw, keys):
    from wholegraph_amd.nn import RGCNConv
    torch.manual_seed(0)
    conv = RGCNConv(32, 16, 535, **kw)
    sd = conv.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == keys
    for name in ("weight", "comp", "root"):
        if name in sd:
            _glorot_ok(sd[name])
    if "bias" in sd:
        assert bool((sd["bias"] == 0).all())
    for name in ("comp", "root", "bias"):
        if name not in keys:
            assert getattr(conv, name) is None
    # a state dict shaped like PyG's loads unchanged
    want = {k: torch.randn(v) for k, v in keys.items()}
    conv.load_state_dict(want)
    for k, v in want.items():
        assert torch.equal(getattr(conv, k).detach(), v)


def test_refusals_and_alias():
    from wholegraph_amd.nn import FastRGCNConv, RGCNConv
    assert FastRGCNConv is RGCNConv
    with pytest.raises(NotImplementedError):
        RGCNConv(8, 8, 3, num_blocks=2)
    with pytest.raises(ValueError, match="aggr"):
        RGCNConv(8, 8, 3, aggr="max")
    conv = RGCNConv(8, 8, 3, is_sorted=True)          # accepted and ignored
    ei = torch.tensor([[0, 1], [1, 0]])
    et = torch.tensor([0, 1])
    with pytest.raises(ValueError, match="featureless"):
        conv(None, ei, et)
    with pytest.raises(ValueError, match="featureless"):
        conv(torch.arange(2), ei, et)


def test_restatement_against_dense_adjacency():
    # 5 nodes, 3 relations: duplicates (0 -> 1 twice, rel 0), a loop (2 -> 2, rel 1), node 3 of in-degree 0, node 4 whose edges
    # all carry relation 2, node 1 with two relations
    pairs = [(0, 1, 0), (0, 1, 0), (2, 1, 0), (3, 1, 1), (2, 2, 1), (0, 2, 1), (1, 4, 2), (3, 4, 2), (0, 0, 2)]
    ei = torch.tensor([[p[0] for p in pairs], [p[1] for p in pairs]])
    et = torch.tensor([p[2] for p in pairs])
    n, R, F, N, B = 5, 3, 4, 3, 2
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n, F, generator=g, dtype=torch.float64)
    basis = torch.randn(B, F, N, generator=g, dtype=torch.float64)
    comp = torch.randn(R, B, generator=g, dtype=torch.float64)
    root = torch.randn(F, N, generator=g, dtype=torch.float64)
    bias = torch.randn(N, generator=g, dtype=torch.float64)
    W = relation_weights(basis, comp)
    for aggr in ("mean", "add"):
        a = dense_relation_adjacency(ei, et, n, R, aggr)
        want = sum(a[r] @ x @ W[r] for r in range(R)) + x @ root + bias
        got = rgcn_forward(x, ei, et, basis, comp, root, bias, aggr=aggr)
        assert torch.allclose(got, want, atol=1e-12), aggr
    # by hand: node 1 under mean = (2 x0 + x2) / 3 @ W0 + x3 @ W1; node 3 = root and bias only; node 4 = (x1 + x3) / 2 @ W2
    got = rgcn_forward(x, ei, et, basis, comp, root, bias)
    assert torch.allclose(got[1], (2 * x[0] + x[2]) / 3 @ W[0] + x[3] @ W[1] + x[1] @ root + bias, atol=1e-12)
    assert torch.allclose(got[3], x[3] @ root + bias, atol=1e-12)
    assert torch.allclose(got[4], (x[1] + x[3]) / 2 @ W[2] + x[4] @ root + bias, atol=1e-12)
    assert torch.allclose(got[2], (x[2] + x[0]) / 2 @ W[1] + x[2] @ root + bias, atol=1e-12)   # the loop is an ordinary edge
    # the magnitude scale bounds the value
    scale = rgcn_forward(x, ei, et, basis, comp, root, bias, abs_terms=True)
    assert bool((got.abs() <= scale + 1e-12).all())
