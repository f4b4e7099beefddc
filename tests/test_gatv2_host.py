"""Host-side checks of wholegraph_amd.nn.GATv2Conv (no GPU): PyG's state-dict keys and shared weights, ``reset_parameters``,
the refused keywords and attention dropout, the refusal of a foreign (x_src, x_dst) pair with self loops, the kernel's shape
domain, the route of CPU tensors, and the layer out of torch ops as well as the float64 restatement the GPU tests measure
against (tests/gatv2_ref.py) against a 4-node graph worked edge by edge (a loop edge, a duplicate edge, a destination without
edges)."""
import math

import pytest
import torch

from gatv2_ref import gatv2_by_hand, gatv2_forward, params_of
from wholegraph_amd.nn import GATv2Conv

KEYS = ["att", "bias", "lin_l.bias", "lin_l.weight", "lin_r.bias", "lin_r.weight"]


def test_state_dict_keys_and_pyg_dict_loads():
    conv = GATv2Conv(8, 4, heads=2)
    assert sorted(conv.state_dict()) == KEYS
    assert conv.att.shape == (1, 2, 4) and conv.bias.shape == (8,)
    assert conv.lin_l.weight.shape == (8, 8) and conv.lin_r.weight.shape == (8, 8) and conv.lin_r is not conv.lin_l
    assert GATv2Conv(8, 4, heads=2, concat=False).bias.shape == (4,)
    assert GATv2Conv((8, 6), 4, heads=2).lin_r.weight.shape == (8, 6)
    nob = GATv2Conv(8, 4, heads=2, bias=False)
    assert nob.bias is None and nob.lin_l.bias is None and sorted(nob.state_dict()) == ["att", "lin_l.weight", "lin_r.weight"]
    want = {"att": torch.randn(1, 2, 4), "bias": torch.randn(8), "lin_l.weight": torch.randn(8, 8), "lin_l.bias": torch.randn(8),
            "lin_r.weight": torch.randn(8, 8), "lin_r.bias": torch.randn(8)}
    conv.load_state_dict(want)
    for k, v in want.items():
        assert torch.equal(conv.state_dict()[k], v), k


def test_share_weights_is_one_module():
    conv = GATv2Conv(8, 4, heads=2, share_weights=True)
    assert conv.lin_r is conv.lin_l
    assert sorted(conv.state_dict()) == KEYS                       # both names, as in PyG
    assert len(list(conv.parameters())) == 4                       # lin_l.weight, lin_l.bias, att, bias


def test_reset_parameters():
    conv = GATv2Conv(6, 4, heads=3)
    before = conv.lin_l.weight.detach().clone()
    with torch.no_grad():
        conv.bias.fill_(5.0)
        conv.lin_r.bias.fill_(5.0)
        conv.att.fill_(9.0)
    conv.reset_parameters()
    assert float(conv.bias.detach().abs().max()) == 0.0 and float(conv.lin_r.bias.detach().abs().max()) == 0.0
    assert float(conv.lin_l.bias.detach().abs().max()) == 0.0
    assert float(conv.att.detach().abs().max()) <= math.sqrt(6.0 / (3 + 4))                 # glorot over [heads, channels]
    assert float(conv.lin_l.weight.detach().abs().max()) <= math.sqrt(6.0 / (6 + 12))       # glorot over [H C, in]
    assert not torch.equal(conv.lin_l.weight.detach(), before)


@pytest.mark.parametrize("kw", ["edge_dim", "fill_value", "residual", "flow"])
def test_unknown_keyword_arguments_are_refused(kw):
    with pytest.raises(TypeError, match=kw):
        GATv2Conv(4, 4, **{kw: 1})


def test_attention_dropout_is_refused_in_training_mode():
    conv = GATv2Conv(4, 4, dropout=0.5)
    x, ei = torch.randn(3, 4), torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(NotImplementedError, match="dropout"):
        conv(x, ei)
    conv.eval()
    assert conv(x, ei).shape == (3, 4)                             # the identity in eval mode


def test_foreign_pair_with_self_loops_is_refused():
    conv = GATv2Conv(4, 4)
    xs, xd, ei = torch.randn(5, 4), torch.randn(3, 4), torch.tensor([[0, 4], [1, 2]])
    with pytest.raises(ValueError, match="add_self_loops=False"):
        conv((xs, xd), ei)
    assert GATv2Conv(4, 4, add_self_loops=False)((xs, xd), ei).shape == (3, 4)
    assert conv((xs, xs[:3]), ei).shape == (3, 4)                  # the sampler layout keeps its self loops


def test_heterogeneous_layer_graph_is_refused():
    from wholegraph_amd import nn
    with pytest.raises(NotImplementedError, match="heterogeneous"):
        GATv2Conv(4, 4)(torch.randn(3, 4), nn.HeteroLayerGraph([], {}, []))


def test_shape_domain(hiplib):
    from wholegraph_amd.nn import gatv2_supported
    for H, C in [(1, 4), (8, 8), (4, 64), (1, 256), (2, 12)]:
        assert gatv2_supported(H, C), (H, C)
    for H, C in [(1, 47), (8, 64), (9, 4), (1, 260)]:
        assert not gatv2_supported(H, C), (H, C)


def test_cpu_tensors_take_the_torch_route():
    conv = GATv2Conv(8, 64, heads=4)                               # inside the kernel's shape domain
    assert conv.route == "torch"
    x, ei = torch.randn(5, 8), torch.tensor([[0, 1, 2], [1, 2, 0]])
    out = conv(x, ei)
    assert out.shape == (5, 256) and not out.is_cuda
    out.sum().backward()                                           # ordinary autograd
    assert conv.att.grad is not None and conv.lin_l.weight.grad is not None


# a 4-node graph: 1 -> 0 twice (a duplicate edge), 2 -> 0, 2 -> 2 (a loop edge), 3 -> 1; node 3 has no incoming edge
EI = torch.tensor([[1, 1, 2, 2, 3], [0, 0, 0, 2, 1]])


def _with_loops(ei, n):
    """Every node's own row as one extra leading neighbour."""
    loops = torch.arange(n)
    return torch.cat([torch.stack([loops, loops]), ei], 1)


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("loops", [False, True])
def test_torch_route_and_restatement_vs_graph_by_hand(concat, share, loops):
    torch.manual_seed(5)
    H, C, F = 2, 3, 4
    conv = GATv2Conv(F, C, heads=H, concat=concat, share_weights=share, add_self_loops=loops).double()
    with torch.no_grad():
        conv.att.mul_(3.0)
        conv.bias.uniform_(-0.5, 0.5)
        conv.lin_l.bias.uniform_(-0.5, 0.5)
        conv.lin_r.bias.uniform_(-0.5, 0.5)
    x = torch.randn(4, F, dtype=torch.float64)
    p = params_of(conv)
    ei = _with_loops(EI, 4) if loops else EI
    hand = gatv2_by_hand(x, None, ei, p, H, concat)
    ref, alpha = gatv2_forward(x, None, ei, p, H, concat, return_alpha=True)
    got = conv(x, EI)
    assert conv.route == "torch"
    assert got.shape == (4, H * C if concat else C)
    assert float((ref - hand).abs().max()) <= 1e-12
    assert float((got.detach() - hand).abs().max()) <= 1e-12
    assert bool(torch.isfinite(got).all())
    if not loops:                                                  # node 3 has no edge: zeros plus bias
        assert torch.equal(got[3].detach(), conv.bias.detach())
        assert torch.equal(ref[3], conv.bias.detach())
    # alpha sums to one per destination and head; the duplicate edge's two entries carry the same weight
    sums = torch.zeros(4, H, dtype=torch.float64).index_add(0, ei[1], alpha)
    has = torch.zeros(4, dtype=torch.bool)
    has[ei[1]] = True
    assert float((sums[has] - 1).abs().max()) <= 1e-12
    k = 4 if loops else 0
    assert torch.equal(alpha[k], alpha[k + 1])
    # relu rides along
    assert torch.equal(conv(x, EI, act=None).relu(), conv(x, _layer_graph(EI, 4), act="relu"))


def _layer_graph(ei, n):
    """The COO graph as a one-hop LayerGraph on the CPU (destinations = all n rows)."""
    from wholegraph_amd import nn
    order = torch.sort(ei[1], stable=True).indices
    rp = torch.zeros(n + 1, dtype=torch.int32)
    rp[1:] = torch.cumsum(torch.bincount(ei[1], minlength=n), 0)
    return nn.LayerGraph([nn.HopGraph(rp, ei[0][order].to(torch.int32), torch.arange(n))])
