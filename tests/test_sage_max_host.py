"""SAGEConv(aggr="max" | "min") on CPU tensors (the torch-ops route) against a float64 restatement, forward and gradients; rows
without neighbours give 0; an unknown aggregator and a max relation inside HeteroConv are refused."""
import pytest
import torch


def ref64(x, w_l, w_r, b, rp, col, self_rows, aggr, relu):
    """The layer in float64, row by row: the extreme over a row's edges (0 for none), lin_l of it, lin_r of the self row."""
    x, red = x.double(), []
    for i in range(rp.shape[0] - 1):
        rows = x[col[int(rp[i]):int(rp[i + 1])].long()]
        red.append((rows.max(0).values if aggr == "max" else rows.min(0).values) if len(rows) else x.new_zeros(x.shape[1]))
    out = torch.stack(red) @ w_l.double().t()
    if w_r is not None:
        out = out + x[self_rows] @ w_r.double().t()
    if b is not None:
        out = out + b.double()
    return out.relu() if relu else out


def _cpu_case(seed, n_dst=9, n_src=14, F=6):
    g = torch.Generator().manual_seed(seed)
    deg = torch.randint(0, 5, (n_dst,), generator=g)
    deg[:2] = torch.tensor([0, 4])
    rp = torch.zeros(n_dst + 1, dtype=torch.int32)
    rp[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, n_src, (int(rp[-1]),), generator=g, dtype=torch.int32)
    return rp, col, torch.randn((n_src, F), generator=g)


@pytest.mark.parametrize("aggr", ["max", "min"])
@pytest.mark.parametrize("relu,root", [(False, True), (True, False)])
def test_cpu_forward_and_gradients_vs_fp64(aggr, relu, root):
    from wholegraph_amd import nn
    rp, col, x = _cpu_case(3)
    n = rp.shape[0] - 1
    torch.manual_seed(1)
    conv = nn.SAGEConv(6, 5, aggr=aggr, root_weight=root)
    x.requires_grad_(True)
    out = conv(x, [rp, col], act="relu" if relu else None)
    assert conv.route == "torch" and out.shape == (n, 5)
    params = [conv.lin_l.weight, conv.lin_l.bias] + ([conv.lin_r.weight] if root else [])
    x64 = x.detach().double().requires_grad_(True)
    p64 = [p.detach().double().requires_grad_(True) for p in params]
    ref = ref64(x64, p64[0], p64[2] if root else None, p64[1], rp, col, torch.arange(n), aggr, relu)
    assert torch.allclose(out.double(), ref, rtol=1e-5, atol=1e-6)
    if not root:      # row 0 has no neighbours: its reduce is 0, the output the bias
        assert torch.allclose(out[0], conv.lin_l.bias.relu() if relu else conv.lin_l.bias)
    w = torch.randn(out.shape, generator=torch.Generator().manual_seed(2))
    got = torch.autograd.grad((out * w).sum(), [x] + params)
    want = torch.autograd.grad((ref * w.double()).sum(), [x64] + p64)
    for a, b in zip(got, want):
        assert torch.allclose(a.double(), b, rtol=1e-5, atol=1e-6)


def test_unknown_aggr_and_hetero_max_are_refused():
    from wholegraph_amd import nn
    with pytest.raises(ValueError, match="'mean', 'sum', 'max' or 'min'"):
        nn.SAGEConv(8, 8, aggr="median")
    with pytest.raises(NotImplementedError, match="max"):
        nn.HeteroConv({("a", "to", "b"): nn.SAGEConv((8, 8), 8, aggr="max")})
