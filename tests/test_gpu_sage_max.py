"""SAGEConv(aggr="max" | "min") on the GPU: the one-kernel layer (wg_sage_max.hip) and its backward against a float64
restatement in torch ops, to the project's bar (_close: |err| <= 1e-5 x the magnitude sum of the terms); launch counts; the tie
rule on both routes; the three graph forms."""
import pytest

from test_gpu_gcn import _close, _edge_index, _hop

pytestmark = pytest.mark.gpu

N_DST, N_SRC = 1003, 1800       # 62 full tiles and one of 11 rows; degrees 0 .. 24 (above the unroll of 8), hubs, loops, duplicates


def red64(x, rp, col, aggr):
    """The element-wise extreme over every row's edges, 0 for a row without any."""
    import torch
    n = rp.shape[0] - 1
    dst = torch.repeat_interleave(torch.arange(n, device=x.device), (rp[1:] - rp[:-1]).long())
    rows = x[col.long()]
    return x.new_zeros((n, x.shape[1])).scatter_reduce(0, dst.unsqueeze(1).expand_as(rows), rows, "a" + aggr, include_self=False)


def lin64(red, xs, w_l, w_r, b, relu=False):
    """lin_l of the reduce, lin_r of the self rows, bias, activation."""
    out = red @ w_l.t() + (0 if b is None else b)
    if w_r is not None:
        out = out + xs @ w_r.t()
    return out.relu() if relu else out


def _abs(*ts):
    return [None if t is None else t.detach().abs() for t in ts]


def _conv(F, N, aggr, root, seed):
    import torch
    from wholegraph_amd import nn
    torch.manual_seed(seed)
    conv = nn.SAGEConv(F, N, aggr=aggr, root_weight=root).cuda()
    with torch.no_grad():
        conv.lin_l.bias.uniform_(-0.5, 0.5)
    return conv


def _params64(conv):
    p = [conv.lin_l.weight, conv.lin_r.weight if conv.lin_r is not None else None, conv.lin_l.bias]
    return [None if t is None else t.detach().double().requires_grad_(True) for t in p]


@pytest.fixture
def launches(monkeypatch):
    """Counts the one-kernel launches (``sage_max_layer_forward`` calls) of the test."""
    from wholegraph_amd import nn
    calls, orig = [], nn.sage_max_layer_forward

    def counted(*a, **kw):
        calls.append(1)
        return orig(*a, **kw)
    monkeypatch.setattr(nn, "sage_max_layer_forward", counted)
    return calls


# (F, N, relu, root_weight): the minimum; tile width 200 -> 208 with padding; full column tiles, no root; the K = 1024 limit;
# F = 516 lies outside the kernel's domain
@pytest.mark.parametrize("F,N,relu,root", [(4, 1, False, True), (100, 47, True, True), (128, 256, False, False),
                                           (512, 256, True, True), (516, 64, False, True)])
@pytest.mark.parametrize("aggr", ["max", "min"])
@pytest.mark.parametrize("ids", [None, "int32", "int64"])
def test_layer_forward_vs_fp64(hiplib, launches, F, N, relu, root, aggr, ids):
    import torch
    from wholegraph_amd import nn
    rp, col, self_rows = _hop(N_DST, N_SRC, 24, seed=F + N)
    hop2 = _hop(37, N_SRC, 9, seed=F)                       # a second hop: one launch each
    table = torch.randn((5000, F), device="cuda")
    x = table[:N_SRC]
    if ids is not None:
        node = torch.randperm(5000, device="cuda")[:N_SRC].to(getattr(torch, ids))
        x = nn.LazyRows(table, node)
    conv = _conv(F, N, aggr, root, seed=N)
    lg = nn.LayerGraph([nn.HopGraph(rp, col, self_rows), nn.HopGraph(*hop2)])
    with torch.no_grad():
        out = conv(x, lg, act="relu" if relu else None)
    in_domain = F != 516
    assert conv.route == ("max_kernel" if in_domain else "torch") and len(launches) == (2 if in_domain else 0)
    xd = (table[node.long()] if ids is not None else x).double()
    w_l, w_r, b = _params64(conv)
    for (r, c, s), rows in (((rp, col, self_rows), slice(0, N_DST)), (hop2, slice(N_DST, N_DST + 37))):
        red = red64(xd, r, c, aggr)
        ref = lin64(red, xd[s], w_l, w_r, b, relu)
        _close(out[rows], ref.detach(), lin64(*_abs(red, xd[s], w_l, w_r, b)), (F, N, aggr, ids))


def _hops_of(sizes, seed):
    """One hop per entry of ``sizes``.  A small hop has degrees 0 .. 70, rows of 0, 1 and 70 edges among them: its transpose
    crosses the 64-entry piece of the input gradient and the 8- and 16-edge unrolls.  0 rows: a hop without rows."""
    import torch
    none = (torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"),
            torch.zeros(0, dtype=torch.int64, device="cuda"))
    return [_hop(n, N_SRC, 24 if n == N_DST else 70, seed=seed + k) if n > 0 else none for k, n in enumerate(sizes)]


# beside the two large shapes: hops of 17, 0 and 33 rows (ragged 16- and 32-row tiles around a hop without rows) with the
# upstream gradient a column-sliced view, rows N + 4 floats apart — without ReLU it reaches the kernels as that view —, and a
# layer graph none of whose hops has rows: no launch, every gradient exact zeros of its input's shape
@pytest.mark.parametrize("F,N,relu,root,sizes,view", [
    pytest.param(100, 47, False, True, (N_DST,), False, id="100-47-False-True"),
    pytest.param(128, 256, True, False, (N_DST,), False, id="128-256-True-False"),
    pytest.param(8, 4, False, True, (17, 0, 33), True, id="8-4-False-True-view"),
    pytest.param(8, 4, True, False, (17, 0, 33), True, id="8-4-True-False-view"),
    pytest.param(8, 4, True, True, (0, 0), False, id="8-4-True-True-no-rows"),
    pytest.param(8, 4, False, False, (0, 0), True, id="8-4-False-False-no-rows-view")])
@pytest.mark.parametrize("aggr", ["max", "min"])
def test_gradients_vs_fp64_autograd(hiplib, launches, F, N, relu, root, sizes, view, aggr):
    """dW_l, dW_r, db, dX; random normal inputs, so ties are duplicate edges of one source (both tie rules give the same sum)."""
    import torch
    hops = _hops_of(sizes, seed=F)
    self_rows, n = torch.cat([h[2] for h in hops]), sum(sizes)
    from wholegraph_amd import nn
    lg = nn.LayerGraph([nn.HopGraph(*h) for h in hops])
    conv = _conv(F, N, aggr, root, seed=F)
    x = torch.randn((N_SRC, F), device="cuda", requires_grad=True)
    g = torch.randn((n, N + 4), device="cuda")[:, :N] if view else torch.randn((n, N), device="cuda")
    params = [p for p in (conv.lin_l.weight, conv.lin_r.weight if root else None, conv.lin_l.bias) if p is not None]
    got = torch.autograd.grad(conv(x, lg, act="relu" if relu else None), [x] + params, g)
    again = torch.autograd.grad(conv(x, lg, act="relu" if relu else None), [x], g)[0]
    assert conv.route == "max_kernel" and len(launches) == 2 * sum(k > 0 for k in sizes)
    assert torch.equal(got[0], again)                       # no atomics, a fixed order: the same bits
    for p in params:                                        # no parameter wants a gradient: no weight-gradient launch, the same dX
        p.requires_grad_(False)
    assert torch.equal(got[0], torch.autograd.grad(conv(x, lg, act="relu" if relu else None), [x], g)[0])
    if n == 0:
        for a, t in zip(got, [x] + params):
            assert a.shape == t.shape and a.dtype == torch.float32 and not bool(a.any())
    x64 = x.detach().double().requires_grad_(True)
    w_l, w_r, b = _params64(conv)
    red = torch.cat([red64(x64, rp, col, aggr) for rp, col, _ in hops])
    ref = lin64(red, x64[self_rows], w_l, w_r, b, relu)
    want = torch.autograd.grad(ref, [x64] + [p for p in (w_l, w_r, b) if p is not None], g.double())
    # the magnitude sums: the same linear maps with |dZ|, |W| and |x| (the selection stays the real one)
    dz = (g.double() * (ref > 0)).abs() if relu else g.double().abs()
    xa = x.detach().double().requires_grad_(True)
    sx = torch.autograd.grad(lin64(torch.cat([red64(xa, rp, col, aggr) for rp, col, _ in hops]), xa[self_rows], *_abs(w_l, w_r), None),
                             xa, dz)[0]
    scales = [sx, dz.t() @ red.detach().abs()] + ([dz.t() @ x64.detach()[self_rows].abs()] if root else []) + [dz.sum(0)]
    for a, b, s, what in zip(got, want, scales, ["dX", "dW_l"] + (["dW_r"] if root else []) + ["db"]):
        _close(a, b, s, (what, F, N, aggr))


@pytest.mark.parametrize("aggr", ["max", "min"])
def test_tie_goes_to_the_lowest_slot_on_both_routes(hiplib, aggr):
    """Sources 0 and 1 hold the same value in columns 0 and 1: the whole gradient goes to the lowest CSR slot, on the kernel
    route and on the torch route (CPU tensors)."""
    import torch
    from wholegraph_amd import nn
    rp = torch.tensor([0, 3, 3, 5], dtype=torch.int32)
    col = torch.tensor([1, 0, 1, 0, 2], dtype=torch.int32)
    x = torch.tensor([[1., 2., 5., 0.], [1., 2., 3., 4.], [1., -7., 8., 4.]])
    torch.manual_seed(0)
    conv = nn.SAGEConv(4, 3, aggr=aggr, root_weight=False)
    g = torch.randn(3, 3)
    dagg = (g.double() @ conv.lin_l.weight.detach().double())
    want, scale = torch.zeros(3, 4, dtype=torch.float64), torch.zeros(3, 4, dtype=torch.float64)
    for i in range(3):
        for f in range(4):
            e = list(range(int(rp[i]), int(rp[i + 1])))
            if e:
                vals = [float(x[col[k], f]) for k in e]
                slot = e[vals.index(max(vals) if aggr == "max" else min(vals))]      # (index: the first, i.e. lowest, slot)
                want[col[slot], f] += dagg[i, f]
                scale[col[slot], f] += (g.double().abs() @ conv.lin_l.weight.detach().double().abs())[i, f]
    for dev, route in (("cuda", "max_kernel"), ("cpu", "torch")):
        conv = conv.to(dev)
        xd = x.to(dev).requires_grad_(True)
        got = torch.autograd.grad(conv(xd, [rp.to(dev), col.to(dev)]), xd, g.to(dev))[0]
        assert conv.route == route
        _close(got, want, scale, (aggr, route))


def test_three_graph_forms_agree(hiplib):
    """COO edge_index, the CSR pair and a LayerGraph over the same hop: the same launches, the same bits."""
    import torch
    from wholegraph_amd import nn
    rp, col, _ = _hop(N_DST, N_SRC, 24, seed=7)
    self_rows = torch.arange(N_DST, device="cuda")
    x = torch.randn((N_SRC, 100), device="cuda")
    conv = _conv(100, 47, "max", True, seed=3)
    with torch.no_grad():
        outs = [conv(xs, graph, act="relu") for xs, graph in (((x, x[:N_DST]), _edge_index(rp, col, self_rows)), (x, [rp, col]),
                                                              (x, nn.LayerGraph([nn.HopGraph(rp, col, self_rows)])))]
        assert conv.route == "max_kernel"
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    w_l, w_r, b = _params64(conv)
    red, xs = red64(x.double(), rp, col, "max"), x.double()[:N_DST]
    _close(outs[0], lin64(red, xs, w_l, w_r, b, True).detach(), lin64(*_abs(red, xs, w_l, w_r, b)), "forms")
