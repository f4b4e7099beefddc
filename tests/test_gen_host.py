"""Host-side checks of wholegraph_amd.nn.GENConv (no GPU, the torch route): forward and every gradient against the float64
restatement (tests/gen_ref.py) on a 4-node graph with a duplicate edge, a loop and a node without edges; t = 0 is the mean; the
state-dict names; route selection and the shape domain; the refusals."""
import pytest
import torch

from gen_ref import gen_forward, params_of
from wholegraph_amd import nn
from wholegraph_amd.nn import GENConv

EI = torch.tensor([[1, 1, 2, 2, 3], [0, 0, 0, 2, 1]])      # 1 -> 0 twice, 2 -> 0, 2 -> 2 (a loop), 3 -> 1; none into 3


@pytest.mark.parametrize("cin,kw", [(6, dict(t=0.7, learn_t=True, bias=True)), (4, dict(t=-2.0, norm="batch", num_layers=3)),
                                    (4, dict(t=50.0, learn_t=True))])
def test_torch_route_forward_and_gradients_vs_restatement(cin, kw):
    torch.manual_seed(5)
    conv = GENConv(cin, 4, **kw).double()
    x = torch.randn(4, cin, dtype=torch.float64, requires_grad=True)
    G = torch.randn(4, 4, dtype=torch.float64)
    perm = torch.tensor([3, 0, 4, 2, 1])                   # COO order is not destination order
    out = conv(x, EI[:, perm], act="relu")
    assert conv.route == "torch"
    (out * G).sum().backward()
    p = {k: v.clone().requires_grad_(True) for k, v in params_of(conv).items()}
    x2, t2 = x.detach().clone().requires_grad_(True), conv.t.detach().clone().requires_grad_(True)
    ref, _ = gen_forward(x2, x2, EI, p, t2, relu=True)
    (ref * G).sum().backward()
    assert float((out.detach() - ref.detach()).abs().max()) <= 1e-10
    for k, v in conv.named_parameters():
        want = t2.grad if k == "aggr_module.t" else p[k].grad
        assert float((v.grad - want).abs().max()) <= 1e-10, k
    assert float((x.grad - x2.grad).abs().max()) <= 1e-10


def test_t_zero_is_the_mean_and_a_row_without_edges_adds_nothing():
    torch.manual_seed(6)
    conv = GENConv(4, 4, t=0.0).double()
    x = torch.randn(4, 4, dtype=torch.float64)
    m = torch.relu(x) + conv.eps
    mean = torch.stack([(2 * m[1] + m[2]) / 3, m[3], m[2], torch.zeros(4, dtype=torch.float64)])
    with torch.no_grad():
        assert float((conv(x, EI) - conv.mlp(mean + x)).abs().max()) <= 1e-12
        assert float((conv((x, None), EI)[:3] - conv.mlp(mean[:3])).abs().max()) <= 1e-12      # (x_src, None): no root term


def test_state_dict_names():
    names = sorted(GENConv((6, 5), 4, learn_t=True, bias=True, norm="layer").state_dict())
    assert names == ["aggr_module.t", "lin_dst.bias", "lin_dst.weight", "lin_src.bias", "lin_src.weight", "mlp.0.bias", "mlp.0.weight",
                     "mlp.1.bias", "mlp.1.weight", "mlp.4.bias", "mlp.4.weight"]
    assert sorted(GENConv(4, 4).state_dict()) == ["mlp.0.weight", "mlp.3.weight"]           # t a float, no lin, no bias
    conv = GENConv(4, 4, expansion=3, num_layers=3)
    assert [tuple(m.weight.shape) for m in conv.mlp if isinstance(m, torch.nn.Linear)] == [(12, 4), (12, 12), (4, 12)]
    assert sorted(conv.state_dict()) == ["mlp.0.weight", "mlp.3.weight", "mlp.6.weight"]


def test_routes_and_shape_domain(hiplib):
    assert nn.gen_layer_supported(256, 256, 256) and nn.gen_layer_supported(20, 36, 20) and nn.gen_layer_supported(4, 8, 4)
    assert nn.gen_layer_supported(32, 1, 0) and not nn.gen_layer_supported(260, 260, 260) and not nn.gen_layer_supported(256, 512, 256)
    assert not nn.gen_layer_supported(18, 36, 18) and not nn.gen_layer_supported(20, 38, 20)
    for kw in (dict(), dict(norm="batch"), dict(num_layers=3)):                            # CPU parameters, float64 parameters
        assert GENConv(48, 32, **kw).route == "torch" and GENConv(32, 32, **kw).double().route == "torch"


def test_refusals(monkeypatch):
    for kw, what in [(dict(msg_norm=True), "msg_norm"), (dict(edge_dim=3), "edge_dim"), (dict(aggr="powermean"), "powermean")]:
        with pytest.raises(NotImplementedError, match=what):
            GENConv(4, 4, **kw)
    for kw in (dict(aggr="max"), dict(norm="instance")):
        with pytest.raises(ValueError):
            GENConv(4, 4, **kw)
    conv, x = GENConv(4, 4), torch.randn(4, 4)
    with pytest.raises(NotImplementedError, match="edge_attr"):
        conv(x, EI, edge_attr=torch.randn(5, 3))
    with pytest.raises(NotImplementedError, match="heterogeneous"):
        conv(x, nn.HeteroLayerGraph.__new__(nn.HeteroLayerGraph))
    hop = nn.HopGraph(torch.tensor([0, 3, 4, 5, 5], dtype=torch.int32), torch.tensor([1, 1, 2, 3, 2], dtype=torch.int32), torch.arange(4))
    with pytest.raises(NotImplementedError, match="pair"):
        conv((x, x), nn.LayerGraph([hop]))
    with pytest.raises(ValueError, match="features"):
        conv(torch.randn(4, 6), EI)
    monkeypatch.setattr(nn, "_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        conv(x, EI)
    assert conv.eval()(x, EI).shape == (4, 4)                                              # inference may be captured
