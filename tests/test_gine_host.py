"""Host-side checks of wholegraph_amd.nn.GINEConv (no GPU, the torch route): forward and every gradient against the float64
restatement of PyG's GINEConv (tests/gine_ref.py) on a 4-node graph with a duplicate edge, a loop and a node without edges; PyG's
state-dict keys; the construction and edge_attr refusals."""
import pytest
import torch

from gine_ref import gine_forward, params_of
from wholegraph_amd.nn import MLP, GINConv, GINEConv

EI = torch.tensor([[1, 1, 2, 2, 3], [0, 0, 0, 2, 1]])      # 1 -> 0 twice, 2 -> 0, 2 -> 2 (a loop), 3 -> 1; none into 3


def _mlp(F, H, N):
    return torch.nn.Sequential(torch.nn.Linear(F, H), torch.nn.ReLU(), torch.nn.Linear(H, N))


@pytest.mark.parametrize("D,train_eps", [(3, True), (None, False)])
def test_torch_route_forward_and_gradients_vs_restatement(D, train_eps):
    torch.manual_seed(5)
    F, H, N = 4, 6, 5
    conv = GINEConv(_mlp(F, H, N), eps=0.3, train_eps=train_eps, edge_dim=D).double()
    assert conv.route == "torch"
    x = torch.randn(4, F, dtype=torch.float64, requires_grad=True)
    ea = torch.randn(5, D or F, dtype=torch.float64, requires_grad=True)
    perm = torch.tensor([3, 0, 4, 2, 1])                   # COO order is not destination order: edge_attr follows edge_index
    G = torch.randn(4, N, dtype=torch.float64)
    out = conv(x, EI[:, perm], edge_attr=ea[perm], act="relu")
    (out * G).sum().backward()
    p = {k: v.clone().requires_grad_(True) for k, v in params_of(conv, [conv.nn[0], conv.nn[2]]).items()}
    x2, ea2 = x.detach().clone().requires_grad_(True), ea.detach().clone().requires_grad_(True)
    ref = gine_forward(x2, x2, EI, ea2, p, relu=True)
    (ref * G).sum().backward()
    assert float((out.detach() - ref.detach()).abs().max()) <= 1e-12
    names = {"nn.0.weight": "W1", "nn.0.bias": "b1", "nn.2.weight": "W2", "nn.2.bias": "b2"}
    names.update({"lin.weight": "We", "lin.bias": "be"} if D else {})
    names.update({"eps": "eps"} if train_eps else {})
    assert sorted(names) == sorted(k for k, _ in conv.named_parameters())
    for k, r in names.items():
        assert float((dict(conv.named_parameters())[k].grad - p[r].grad).abs().max()) <= 1e-12, k
    assert float((x.grad - x2.grad).abs().max()) <= 1e-12 and float((ea.grad - ea2.grad).abs().max()) <= 1e-12


def test_state_dict_keys_are_pygs():
    conv = GINEConv(_mlp(8, 4, 4), edge_dim=3)
    assert sorted(conv.state_dict()) == ["eps", "lin.bias", "lin.weight", "nn.0.bias", "nn.0.weight", "nn.2.bias", "nn.2.weight"]
    assert conv.lin.weight.shape == (8, 3) and "eps" not in dict(conv.named_parameters())
    conv.load_state_dict({k: torch.randn_like(v) for k, v in conv.state_dict().items()}, strict=True)
    assert "eps" in dict(GINEConv(_mlp(8, 4, 4), train_eps=True).named_parameters())
    assert not [k for k in GINEConv(_mlp(8, 4, 4)).state_dict() if k.startswith("lin")]
    assert GINEConv(MLP([8, 4, 4]), edge_dim=2).lin.weight.shape == (8, 2)                # channel_list[0] of an MLP


def test_refusals():
    x, ea = torch.randn(4, 4), torch.randn(5, 3)
    conv = GINEConv(_mlp(4, 4, 4), edge_dim=3)
    for bad, what in [(None, "needs edge_attr"), (torch.ones(5, 3, dtype=torch.int64), "floating"), (torch.randn(5, 2), r"\[E, 3\]"),
                      (torch.randn(4, 3), "4 rows for 5 edges"), (torch.randn(5), r"\[E, 3\]")]:
        with pytest.raises(ValueError, match=what):
            conv(x, EI, edge_attr=bad)
    with pytest.raises(ValueError, match=r"\[E, 4\]"):
        GINEConv(_mlp(4, 4, 4))(x, EI, edge_attr=ea)                                       # no lin: the rows are as wide as x
    with pytest.raises(TypeError, match="edge_attr="):
        conv(x, EI, ea)
    assert GINEConv(_mlp(4, 4, 4), edge_dim=1)(x, EI, edge_attr=torch.randn(5)).shape == (4, 4)     # [E] with edge_dim == 1
    with pytest.raises(ValueError, match="infer"):
        GINEConv(torch.nn.Sequential(torch.nn.ReLU(), torch.nn.Linear(4, 4)), edge_dim=3)
    for bad in (0, True, 2.0):
        with pytest.raises(ValueError, match="edge_dim"):
            GINEConv(_mlp(4, 4, 4), edge_dim=bad)
    with pytest.raises(TypeError, match="edge_dim"):
        GINConv(_mlp(4, 4, 4), edge_dim=3)                                                 # the plain layer still refuses it
    with pytest.raises(NotImplementedError, match="pair"):
        from wholegraph_amd.nn import HopGraph, LayerGraph
        hop = HopGraph(torch.tensor([0, 3, 4, 5, 5], dtype=torch.int32), torch.tensor([1, 1, 2, 3, 2], dtype=torch.int32), torch.arange(4))
        conv((x, x), LayerGraph([hop]), edge_attr=ea)


def test_shape_domain(hiplib):
    from wholegraph_amd.nn import gine_layer_supported
    assert gine_layer_supported(256, 256, 256, 16) and gine_layer_supported(20, 36, 12, 3) and gine_layer_supported(48, 16, 8, 0)
    assert not gine_layer_supported(16, 8, 8, 17) and not gine_layer_supported(18, 8, 8, 3) and not gine_layer_supported(16, 6, 8, 3)
