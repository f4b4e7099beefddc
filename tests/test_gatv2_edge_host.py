"""Host-side checks of wholegraph_amd.nn.GATv2EdgeConv (no GPU, the torch route): forward and every gradient against the float64
restatement of PyG's GATv2Conv(edge_dim) (tests/gatv2_edge_ref.py) on the 4-node graph of test_gatv2_host.py (a duplicate edge, a
sampled loop, a node without edges) with both kinds of fill row, PyG's state-dict keys, and the refusals."""
import pytest
import torch

from gatv2_edge_ref import edge_params_of, gatv2_edge_forward, with_loops
from wholegraph_amd.nn import GATv2Conv, GATv2EdgeConv

EI = torch.tensor([[1, 1, 2, 2, 3], [0, 0, 0, 2, 1]])      # 1 -> 0 twice, 2 -> 0, 2 -> 2 (a sampled loop), 3 -> 1; none into 3


@pytest.mark.parametrize("loops,fill", [(False, "mean"), (True, "mean"), (True, 0.25)])
@pytest.mark.parametrize("concat,share", [(True, False), (False, True)])
def test_torch_route_forward_and_gradients_vs_restatement(loops, fill, concat, share):
    torch.manual_seed(3)
    H, C, F, D = 2, 3, 4, 5
    conv = GATv2EdgeConv(F, C, D, heads=H, concat=concat, share_weights=share, add_self_loops=loops, fill_value=fill).double()
    with torch.no_grad():
        conv.att.mul_(3.0)
        for b in (conv.bias, conv.lin_l.bias, conv.lin_r.bias):
            b.uniform_(-0.5, 0.5)
    assert conv.route == "torch"
    x = torch.randn(4, F, dtype=torch.float64, requires_grad=True)
    ea = torch.randn(5, D, dtype=torch.float64, requires_grad=True)
    perm = torch.tensor([3, 0, 4, 2, 1])                   # COO order is not destination order: edge_attr follows edge_index
    G = torch.randn(4, H * C if concat else C, dtype=torch.float64)
    out = conv(x, EI[:, perm], edge_attr=ea[perm], act="relu")
    (out * G).sum().backward()
    p = {k: v.clone().requires_grad_(True) for k, v in edge_params_of(conv).items()}
    if share:
        p["Wr"], p["br"] = p["Wl"], p["bl"]
    x2, ea2 = x.detach().clone().requires_grad_(True), ea.detach().clone().requires_grad_(True)
    ei, rows = with_loops(EI, ea2, torch.arange(4), fill) if loops else (EI, ea2)
    ref = gatv2_edge_forward(x2, ei, rows, p, H, concat, relu=True)
    (ref * G).sum().backward()
    assert float((out.detach() - ref.detach()).abs().max()) <= 1e-12
    if loops and fill == "mean":                           # node 3 has no sampled edge: its loop's row is zeros, alpha = 1
        alone = conv.lin_l(x[3:4]).view(H, C)
        want = alone.reshape(-1) if concat else alone.mean(0)
        assert float((out[3] - torch.relu(want + conv.bias)).detach().abs().max()) <= 1e-12
    got = {"lin_l.weight": "Wl", "lin_l.bias": "bl", "lin_edge.weight": "We", "att": "att", "bias": "bias"}
    if not share:
        got.update({"lin_r.weight": "Wr", "lin_r.bias": "br"})
    for k, r in got.items():
        assert float((dict(conv.named_parameters())[k].grad - p[r].grad).abs().max()) <= 1e-12, k
    assert float((x.grad - x2.grad).abs().max()) <= 1e-12 and float((ea.grad - ea2.grad).abs().max()) <= 1e-12


def test_state_dict_keys_are_pygs():
    conv = GATv2EdgeConv(8, 4, 3, heads=2)
    assert sorted(conv.state_dict()) == ["att", "bias", "lin_edge.weight", "lin_l.bias", "lin_l.weight", "lin_r.bias", "lin_r.weight"]
    assert conv.lin_edge.weight.shape == (8, 3) and conv.lin_edge.bias is None
    assert float(conv.lin_edge.weight.detach().abs().max()) <= (6.0 / 11) ** 0.5          # glorot over [H C, D]
    conv.load_state_dict({k: torch.randn_like(v) for k, v in conv.state_dict().items()}, strict=True)


def test_refusals():
    x, ea = torch.randn(4, 4), torch.randn(5, 3)
    conv = GATv2EdgeConv(4, 4, 3)
    for bad, what in [(None, "needs edge_attr"), (torch.ones(5, 3, dtype=torch.int64), "floating"), (torch.randn(5, 2), r"\[E, 3\]"),
                      (torch.randn(4, 3), "4 rows for 5 edges"), (torch.randn(5), r"\[E, 3\]")]:
        with pytest.raises(ValueError, match=what):
            conv(x, EI, edge_attr=bad)
    with pytest.raises(TypeError, match="edge_attr="):
        conv(x, EI, ea)
    assert GATv2EdgeConv(4, 4, 1)(x, EI, edge_attr=torch.randn(5)).shape == (4, 4)         # [E] with edge_dim == 1
    for fill in ("add", None, True):
        with pytest.raises(ValueError, match="fill_value"):
            GATv2EdgeConv(4, 4, 3, fill_value=fill)
    with pytest.raises(TypeError, match="edge_dim"):
        GATv2Conv(4, 4, edge_dim=3)                                                        # the plain layer still refuses it
    with pytest.raises(NotImplementedError, match="dropout"):
        GATv2EdgeConv(4, 4, 3, dropout=0.5)(x, EI, edge_attr=ea)


def test_shape_domain(hiplib):
    from wholegraph_amd.nn import gatv2_edge_supported
    assert gatv2_edge_supported(4, 64, 16) and gatv2_edge_supported(2, 12, 1)
    assert not gatv2_edge_supported(1, 16, 17) and not gatv2_edge_supported(1, 16, 0) and not gatv2_edge_supported(1, 47, 4)
