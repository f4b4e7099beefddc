"""A second backward through a one-kernel layer: the tensors the forward kept for the backward (aggregates, activations, per-edge
coefficients, input rows) are released by the first backward pass whatever ``retain_graph`` says, so the second one raises a
RuntimeError that says so — for every layer — and a fresh forward and backward afterwards gives the first pass's gradients bit
for bit (these backward passes have no atomics).  Over the two-hop layer graph of test_gpu_layer_empty_hop.py at F = 64, output
width 16: a shape every one of these layers has in its kernel's domain."""
import pytest

from layer_graphs import empty_hop_graph

pytestmark = pytest.mark.gpu

N_SRC, F = 300, 64


def _sage(nn, torch, lg, E, g):
    return nn.SAGEConv(F, 16), (), "_SageLayerBackward"


def _gcn(nn, torch, lg, E, g):
    lg.degree_source = lambda: (lg.hops, [-1, -1], N_SRC)
    return nn.GCNConv(F, 16), (), "_GcnLayerBackward"


def _rgcn(nn, torch, lg, E, g):
    return nn.RGCNConv(F, 16, 3, num_bases=2), (torch.randint(0, 3, (E,), generator=g, device="cuda"),), "_RgcnLayerBackward"


def _transformer(nn, torch, lg, E, g):
    return nn.TransformerConv(F, 8, heads=2), (), "_TconvLayerBackward"


def _gin(nn, torch, lg, E, g):
    mlp = torch.nn.Sequential(torch.nn.Linear(F, 16), torch.nn.ReLU(), torch.nn.Linear(16, 16))
    return nn.GINConv(mlp), (), "_GinLayerBackward"


@pytest.mark.parametrize("make", [_sage, _gcn, _rgcn, _transformer, _gin], ids=lambda f: f.__name__.strip("_"))
def test_second_backward_raises_and_a_fresh_pass_repeats_the_gradients(hiplib, make):
    import torch
    from wholegraph_amd import nn
    lg, ei, _ = empty_hop_graph(N_SRC, seed=3)
    g = torch.Generator(device="cuda").manual_seed(5)
    torch.manual_seed(0)
    conv, extra, function = make(nn, torch, lg, ei.shape[1], g)
    conv = conv.cuda()
    x = torch.randn((N_SRC, F), generator=g, device="cuda").requires_grad_(True)
    leaves = [x] + list(conv.parameters())

    out = conv(x, lg, *extra)
    assert out.shape == (120, 16)
    assert type(out.grad_fn).__name__ == function, "the layer's own autograd Function did not run"      # (a)
    out.sum().backward(retain_graph=True)                                                               # (b)
    assert all(t.grad is not None for t in leaves)
    first = [t.grad.clone() for t in leaves]
    with pytest.raises(RuntimeError, match="a second time"):                                            # (c)
        out.sum().backward()
    for t in leaves:                                                                                    # (d)
        t.grad = None
    conv(x, lg, *extra).sum().backward()
    for t, want in zip(leaves, first):
        assert t.grad is not None and torch.equal(t.grad, want)
