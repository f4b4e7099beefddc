"""Host-side checks of wholegraph_amd.nn.GINConv and global_add_pool (no GPU): PyG's state-dict keys (``eps`` as a buffer or a
Parameter, ``nn.*``), ``reset_parameters``, the refusal of unknown keyword arguments, the route every ``nn`` form selects, the
kernel's shape domain at its edges, and the layer on CPU tensors as well as the float64 restatement the GPU tests measure against
(tests/gin_ref.py) against a 4-node graph computed by hand (a loop edge and a duplicate edge, both summed)."""
import pytest
import torch

from gin_ref import gin_aggregate, gin_forward
from wholegraph_amd.nn import GINConv, global_add_pool

Seq, Lin, ReLU = torch.nn.Sequential, torch.nn.Linear, torch.nn.ReLU


def test_state_dict_keys_and_pyg_dict_loads():
    conv = GINConv(Seq(Lin(8, 16), ReLU(), Lin(16, 4)))
    assert sorted(conv.state_dict()) == ["eps", "nn.0.bias", "nn.0.weight", "nn.2.bias", "nn.2.weight"]
    assert "eps" in dict(conv.named_buffers()) and "eps" not in dict(conv.named_parameters())
    assert conv.eps.shape == (1,) and float(conv.eps.detach()) == 0.0
    conv = GINConv(Seq(Lin(8, 16), ReLU(), Lin(16, 4)), eps=0.25, train_eps=True)
    assert sorted(conv.state_dict()) == ["eps", "nn.0.bias", "nn.0.weight", "nn.2.bias", "nn.2.weight"]
    assert isinstance(conv.eps, torch.nn.Parameter) and conv.eps.requires_grad and float(conv.eps.detach()) == 0.25
    want = {"eps": torch.tensor([0.75]), "nn.0.weight": torch.randn(16, 8), "nn.0.bias": torch.randn(16),
            "nn.2.weight": torch.randn(4, 16), "nn.2.bias": torch.randn(4)}
    conv.load_state_dict(want)
    assert float(conv.eps.detach()) == 0.75 and torch.equal(conv.nn[2].weight.detach(), want["nn.2.weight"])


def test_reset_parameters():
    conv = GINConv(Seq(Lin(4, 4), ReLU(), Lin(4, 4)), eps=0.5, train_eps=True)
    before = conv.nn[0].weight.detach().clone()
    with torch.no_grad():
        conv.eps.fill_(3.0)
        conv.nn[2].bias.fill_(100.0)
    conv.reset_parameters()
    assert float(conv.eps.detach()) == 0.5
    assert float(conv.nn[2].bias.detach().abs().max()) <= 0.5         # Linear's own initialisation: |b| <= 1 / sqrt(4)
    assert not torch.equal(conv.nn[0].weight.detach(), before)


def test_unknown_keyword_arguments_are_refused():
    with pytest.raises(TypeError, match="unsupported"):
        GINConv(Lin(4, 4), aggr="mean")
    with pytest.raises(TypeError, match="unsupported"):
        GINConv(Lin(4, 4), flow="target_to_source")
    with pytest.raises(TypeError):
        GINConv(lambda t: t)


def test_routes_and_shape_domain(hiplib):
    from wholegraph_amd.nn import gin_layer_supported
    assert GINConv(Seq(Lin(100, 256), ReLU(), Lin(256, 47))).route == "mlp"
    assert GINConv(Seq(Lin(100, 256), ReLU(inplace=True), Lin(256, 256))).route == "mlp"
    assert GINConv(Lin(64, 32)).route == "linear"
    assert GINConv(Seq(Lin(64, 32))).route == "linear"
    assert GINConv(Seq(Lin(64, 32), ReLU())).route == "linear"
    assert GINConv(Seq(Lin(64, 32), torch.nn.BatchNorm1d(32), ReLU(), Lin(32, 8))).route == "linear"
    assert GINConv(Seq(Lin(64, 32), ReLU(), Lin(32, 8), ReLU())).route == "linear"
    assert GINConv(Seq(Lin(64, 30), ReLU(), Lin(30, 8))).route == "linear"       # W2's rows are not 16-B aligned
    assert GINConv(Seq(Lin(64, 32), ReLU(), Lin(32, 300))).route == "linear"     # the second product lies outside the domain
    assert GINConv(Seq(Lin(300, 64), ReLU(), Lin(64, 64))).route == "aggregate"
    assert GINConv(Seq(Lin(66, 64), ReLU(), Lin(64, 64))).route == "aggregate"
    assert GINConv(Seq(ReLU(), Lin(64, 64))).route == "aggregate"
    assert GINConv(torch.nn.Identity()).route == "aggregate"
    plan = GINConv(Seq(Lin(64, 32), torch.nn.BatchNorm1d(32), ReLU(), Lin(32, 8)))._plan()
    assert plan[2] is False and [type(m).__name__ for m in plan[4]] == ["BatchNorm1d", "ReLU", "Linear"]
    assert gin_layer_supported(256, 256, 256) and gin_layer_supported(4, 4, 1) and gin_layer_supported(100, 256, 47)
    assert gin_layer_supported(4, 1, 0) and gin_layer_supported(256, 255, 0)
    for F, H, N in [(260, 64, 64), (0, 64, 64), (6, 64, 64), (64, 260, 64), (64, 64, 257), (64, 30, 8), (64, 0, 0), (64, 257, 0)]:
        assert not gin_layer_supported(F, H, N), (F, H, N)


# 4 nodes, F = 2; edges src -> dst: 0 -> 1 twice (a duplicate), 1 -> 1 (a loop), 2 -> 0, 3 -> 2, 1 -> 2; node 3 has no in-edge
X = [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7.0, 8.0]]
EI = [[0, 0, 1, 2, 3, 1], [1, 1, 1, 0, 2, 2]]
SUMS = [[5.0, 6.0], [5.0, 8.0], [10.0, 12.0], [0.0, 0.0]]          # dst 1: x0 + x0 + x1


def _identity_conv(**kw):
    lin = Lin(2, 2)
    with torch.no_grad():
        lin.weight.copy_(torch.eye(2))
        lin.bias.zero_()
    return GINConv(lin, **kw)


def _hand(eps):
    return torch.tensor([[s + (1 + eps) * v for s, v in zip(srow, xrow)] for srow, xrow in zip(SUMS, X)])


@pytest.mark.parametrize("eps", [0.0, 0.5])
def test_cpu_layer_and_reference_against_hand_numbers(eps):
    x, ei = torch.tensor(X), torch.tensor(EI)
    want = _hand(eps)
    got = _identity_conv(eps=eps)(x, ei)
    assert torch.allclose(got, want, atol=1e-6), got
    assert torch.allclose(gin_aggregate(x, ei, eps), want.double(), atol=1e-12)
    # the GIN paper's MLP with weights chosen by hand
    mlp = Seq(Lin(2, 2), ReLU(), Lin(2, 1))
    with torch.no_grad():
        mlp[0].weight.copy_(torch.tensor([[1.0, 0.0], [0.0, -1.0]]))
        mlp[0].bias.copy_(torch.tensor([0.0, 10.0]))
        mlp[2].weight.copy_(torch.tensor([[1.0, 1.0]]))
        mlp[2].bias.fill_(0.5)
    hidden = torch.stack([want[:, 0], (10.0 - want[:, 1]).clamp(min=0)], 1)
    out = hidden.sum(1, keepdim=True) + 0.5
    if eps == 0.0:
        assert out.flatten().tolist() == [8.5, 8.5, 15.5, 9.5]
    got = GINConv(mlp, eps=eps)(x, ei)
    assert torch.allclose(got, out, atol=1e-6), got
    ref = gin_forward(x, ei, mlp[0].weight.detach(), mlp[0].bias.detach(), mlp[2].weight.detach(), mlp[2].bias.detach(), eps=eps)
    assert torch.allclose(ref, out.double(), atol=1e-12)
    got = GINConv(mlp, eps=eps)(x, ei, act="relu")
    assert torch.allclose(got, out.clamp(min=0), atol=1e-6)
    scale = gin_forward(-x, ei, -mlp[0].weight.detach(), mlp[0].bias.detach(), mlp[2].weight.detach(), -mlp[2].bias.detach(),
                        eps=eps, abs_terms=True)
    assert torch.allclose(scale, (want[:, :1] + want[:, 1:] + 10.0 + 0.5).double(), atol=1e-12)


def test_cpu_pair_forms():
    x, ei = torch.tensor(X), torch.tensor(EI)
    got = _identity_conv(eps=0.5)((x, None), ei)               # no root term; as many rows as the edges reach
    assert torch.allclose(got, torch.tensor(SUMS[:3]), atol=1e-6), got
    assert torch.allclose(gin_aggregate(x, ei, 0.5, root=False), torch.tensor(SUMS[:3]).double(), atol=1e-12)
    x_dst = torch.tensor([[10.0, 20.0], [30.0, 40.0], [50.0, 60.0], [70.0, 80.0], [90.0, 100.0]])   # more destinations than sources
    got = _identity_conv(eps=0.5)((x, x_dst), ei)
    want = torch.tensor(SUMS + [[0.0, 0.0]]) + 1.5 * x_dst
    assert torch.allclose(got, want, atol=1e-5), got
    assert torch.allclose(gin_aggregate(x, ei, 0.5, x_dst=x_dst), want.double(), atol=1e-12)


def test_cpu_train_eps_gradient():
    x, ei = torch.tensor(X), torch.tensor(EI)
    conv = _identity_conv(eps=0.5, train_eps=True)
    conv(x, ei).sum().backward()
    assert float(conv.eps.grad) == pytest.approx(float(x.sum()))


def test_global_add_pool_cpu():
    x = torch.tensor(X, requires_grad=True)
    out = global_add_pool(x, torch.tensor([0, 0, 2, 2]), size=4)          # graph 1 is empty, graph 3 lies past batch.max()
    assert out.tolist() == [[4.0, 6.0], [0.0, 0.0], [12.0, 14.0], [0.0, 0.0]]
    (out * torch.tensor([[1.0], [2.0], [3.0], [4.0]])).sum().backward()
    assert x.grad.tolist() == [[1.0, 1.0], [1.0, 1.0], [3.0, 3.0], [3.0, 3.0]]
    out = global_add_pool(torch.tensor(X), torch.tensor([2, 0, 2, 0]))    # unsorted
    assert out.tolist() == [[10.0, 12.0], [0.0, 0.0], [6.0, 8.0]]
    assert global_add_pool(torch.tensor(X), None).tolist() == [[16.0, 20.0]]
