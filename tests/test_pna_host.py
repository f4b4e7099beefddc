"""Host-side checks of wholegraph_amd.nn.PNAConv (no GPU, the torch route): forward and every gradient against the float64
restatement (tests/pna_ref.py) on a 4-node graph with a duplicate edge (a tie of min and max), a loop and a node without edges; the
state-dict names; what the constructor selects; the refusals."""
import pytest
import torch

from pna_ref import params_of, pna_forward
from wholegraph_amd import nn
from wholegraph_amd.nn import PNAConv

EI = torch.tensor([[1, 1, 2, 2, 3], [0, 0, 0, 2, 1]])      # 1 -> 0 twice, 2 -> 0, 2 -> 2 (a loop), 3 -> 1; none into 3
DEG = torch.tensor([1, 2, 0, 1])                           # the in-degree histogram of EI
ALL = ["sum", "mean", "min", "max", "var", "std"]
S3 = ["identity", "amplification", "attenuation"]


@pytest.mark.parametrize("aggr,scalers,kw", [(ALL, S3, dict()), (["max", "std"], ["linear", "inverse_linear"], dict(train_norm=True)),
                                             (["mean", "min", "max", "std"], S3, dict(towers=2, divide_input=True, pre_layers=2, post_layers=2)),
                                             (["sum", "var"], ["attenuation"], dict(towers=2))])
def test_torch_route_forward_and_gradients_vs_restatement(aggr, scalers, kw):
    torch.manual_seed(5)
    conv = PNAConv(4, 6, aggr, scalers, DEG, **kw).double()
    x = torch.randn(4, 4, dtype=torch.float64, requires_grad=True)
    G = torch.randn(4, 6, dtype=torch.float64)
    perm = torch.tensor([3, 0, 4, 2, 1])                   # COO order is not destination order; a row's edges keep theirs
    out = conv(x, EI[:, perm], act="relu")
    assert conv.route == "torch"
    (out * G).sum().backward()
    p = {k: v.clone().requires_grad_(True) for k, v in params_of(conv).items()}
    x2 = x.detach().clone().requires_grad_(True)
    avg = (p.pop("aggr_module.avg_deg_lin"), p.pop("aggr_module.avg_deg_log")) if kw.get("train_norm") else \
        (float(conv.aggr_module.avg_deg_lin), float(conv.aggr_module.avg_deg_log))
    p.pop("aggr_module.avg_deg_exp", None)
    ref, _ = pna_forward(x2, x2, EI[:, perm], p, aggr, scalers, *avg, towers=kw.get("towers", 1), divide_input=kw.get("divide_input", False),
                         relu=True)
    (ref * G).sum().backward()
    assert float((out.detach() - ref.detach()).abs().max()) <= 1e-10
    named = dict(conv.named_parameters())
    for k, v in p.items():
        assert float((named[k].grad - v.grad).abs().max()) <= 1e-10, k
    if kw.get("train_norm"):
        assert abs(float(named["aggr_module.avg_deg_log"].grad or 0.0) - float(avg[1].grad or 0.0)) <= 1e-10
        assert abs(float(named["aggr_module.avg_deg_lin"].grad) - float(avg[0].grad)) <= 1e-10
    assert float((x.grad - x2.grad).abs().max()) <= 1e-10


def test_degree_averages_and_state_dict_names():
    conv = PNAConv(4, 6, ["mean"], ["identity"], DEG, towers=2, pre_layers=2)
    assert abs(float(conv.aggr_module.avg_deg_lin) - 5 / 4) < 1e-6                       # (0 + 2 + 0 + 3) / 4
    assert abs(float(conv.aggr_module.avg_deg_log) - (2 * 0.6931471805599453 + 1.3862943611198906) / 4) < 1e-6
    assert sorted(conv.state_dict()) == sorted(
        ["aggr_module.avg_deg_%s" % k for k in ("lin", "log", "exp")] + ["lin.weight", "lin.bias"]
        + ["%s.%d.%d.%s" % (n, t, k, w) for n, ks in (("pre_nns", (0, 2)), ("post_nns", (0,))) for t in (0, 1) for k in ks for w in ("weight", "bias")])
    one = PNAConv(8, 12, ALL, S3, DEG)
    assert tuple(one.pre_nns[0][0].weight.shape) == (8, 16) and tuple(one.post_nns[0][0].weight.shape) == (12, 19 * 8)
    assert tuple(PNAConv(8, 12, ALL, S3, DEG, towers=2, divide_input=True).post_nns[1][0].weight.shape) == (6, 19 * 4)


def test_plan_per_constructor(hiplib):
    plan = lambda cin, cout, **kw: PNAConv(cin, cout, ALL, S3, DEG, **kw)._plan_shapes()      # noqa: E731  (parameters on the device)
    assert plan(256, 256) == "layer" and plan(4, 8) == "layer" and plan(20, 36) == "layer"
    assert plan(16, 32, towers=4) == "aggregate" and plan(32, 32, post_layers=2) == "aggregate" and plan(32, 30) == "aggregate"
    assert plan(64, 512) == "aggregate" and plan(128, 64, towers=4, divide_input=True) == "aggregate"
    assert plan(260, 64) == "torch" and plan(18, 16) == "torch" and plan(128, 64, towers=4) == "torch"      # y 512 wide
    assert plan(32, 32, pre_layers=2) == "torch" and plan(32, 32, train_norm=True) == "torch"
    assert PNAConv(32, 32, ALL, S3, DEG).route == "torch" and PNAConv(32, 32, ALL, S3, DEG).double().route == "torch"      # CPU, float64
    assert nn.pna_row_tiles(256, 6, 256) == 1 and nn.pna_row_tiles(64, 6, 48) == 4
    assert nn.pna_row_tiles(128, 6, 128) == 2 and nn.pna_row_tiles(64, 4, 256) == 4


def test_refusals(monkeypatch):
    with pytest.raises(NotImplementedError, match="edge_dim"):
        PNAConv(4, 4, ALL, S3, DEG, edge_dim=3)
    for aggr, scalers in ((["median"], S3), (ALL, ["exponential"]), ([], S3)):
        with pytest.raises(ValueError):
            PNAConv(4, 4, aggr, scalers, DEG)
    conv, x = PNAConv(4, 4, ALL, S3, DEG), torch.randn(4, 4)
    with pytest.raises(NotImplementedError, match="edge_attr"):
        conv(x, EI, edge_attr=torch.randn(5, 3))
    with pytest.raises(NotImplementedError, match="heterogeneous"):
        conv(x, nn.HeteroLayerGraph.__new__(nn.HeteroLayerGraph))
    hop = nn.HopGraph(torch.tensor([0, 3, 4, 5, 5], dtype=torch.int32), torch.tensor([1, 1, 2, 3, 2], dtype=torch.int32), torch.arange(4))
    with pytest.raises(NotImplementedError, match="pair"):
        conv((x, x), nn.LayerGraph([hop]))
    with pytest.raises(NotImplementedError, match="LazyRows"):
        conv(nn.LazyRows(torch.randn(9, 4, requires_grad=True), torch.arange(4)), nn.LayerGraph([hop]))
    with pytest.raises(ValueError, match="features"):
        conv(torch.randn(4, 6), EI)
    with pytest.raises(ValueError, match="destination"):
        conv((x, None), EI)
    monkeypatch.setattr(nn, "_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        conv(x, EI)
    assert conv.eval()(x, EI).shape == (4, 4)                                              # inference may be captured
