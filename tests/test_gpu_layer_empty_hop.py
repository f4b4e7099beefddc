"""A call-group LayerGraph in which one hop has no edges, through the one-kernel GCN (with edge weights), RGCN and transformer
layers, forward and backward: the hop's rows are those of a destination without neighbours, and its transpose (the input
gradient's graph) is the empty-hop branch of ``HopGraph.transposed``.  Against the float64 restatements of the PyG layers over
the edge_index of the whole layer graph (destinations = input rows ``self_rows``)."""
import pytest

from gcn_ref import gcn_forward
from layer_graphs import empty_hop_graph as _graph
from rgcn_ref import rgcn_forward
from transformer_ref import params_of, transformer_forward

pytestmark = pytest.mark.gpu


def _check(got, ref, what):
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, what
    assert float((got - ref).abs().max()) <= 1e-4 * max(1.0, float(ref.abs().max())), what


def test_empty_hop_forward_backward(hiplib):
    import torch
    from wholegraph_amd import nn
    n_src, F = 300, 32
    lg, ei, dst = _graph(n_src, seed=3)
    E = ei.shape[1]
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((n_src, F), generator=g, device="cuda")

    # GCN with edge weights (per hop; the empty hop's are empty)
    torch.manual_seed(0)
    conv = nn.GCNConv(F, 24).cuda()
    w = torch.rand(E, generator=g, device="cuda") + 0.5
    weights = [w, torch.zeros(0, device="cuda")]
    lg.degree_source = lambda: (lg.hops, [-1, -1], n_src)
    lg._gcn_edge_weights = weights
    xg = x.clone().requires_grad_(True)
    out = conv._forward_layer(xg, lg, edge_weights=weights)
    out.sum().backward()
    xr = x.double().requires_grad_(True)
    wr, br = conv.lin.weight.detach().double().requires_grad_(True), conv.bias.detach().double().requires_grad_(True)
    ref = gcn_forward(xr, ei, wr, br, edge_weight=w.double())[dst]
    ref.sum().backward()
    _check(out, ref, "gcn out")
    for got, want, what in ((xg.grad, xr.grad, "gcn dx"), (conv.lin.weight.grad, wr.grad, "gcn dW"), (conv.bias.grad, br.grad, "gcn db")):
        _check(got, want, what)

    # RGCN with bases
    R = 3
    et = torch.randint(0, R, (E,), generator=g, device="cuda")
    torch.manual_seed(1)
    conv = nn.RGCNConv(F, 24, R, num_bases=2).cuda()
    xg = x.clone().requires_grad_(True)
    out = conv(xg, lg, et)
    out.sum().backward()
    xr = x.double().requires_grad_(True)
    p = {k: getattr(conv, k).detach().double().requires_grad_(True) for k in ("weight", "comp", "root", "bias")}
    ref = rgcn_forward(xr, ei, et, **p)[dst]
    ref.sum().backward()
    _check(out, ref, "rgcn out")
    _check(xg.grad, xr.grad, "rgcn dx")
    for k in p:
        _check(getattr(conv, k).grad, p[k].grad, "rgcn d" + k)

    # TransformerConv with edge attributes
    torch.manual_seed(2)
    conv = nn.TransformerConv(F, 8, heads=2, edge_dim=3).cuda()
    ea = torch.randn((E, 3), generator=g, device="cuda")
    xg = x.clone().requires_grad_(True)
    out, alpha = conv(xg, lg, ea, return_attention_weights=True)
    out.sum().backward()
    xr = x.double().requires_grad_(True)
    ref, ra = transformer_forward(xr, None, ei, params_of(conv), 2, True, ea, return_alpha=True)
    ref = ref[dst]
    ref.sum().backward()
    _check(out, ref, "transformer out")
    _check(alpha, ra, "transformer alpha")
    _check(xg.grad, xr.grad, "transformer dx")
