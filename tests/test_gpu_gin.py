"""GPU parity of wholegraph_amd.nn.GINConv and global_add_pool (csrc/wg_gin.hip): the one-kernel layer with its MLP, the
one-product and aggregate-only routes, the three graph forms, the bipartite pair, every gradient (dW1, db1, dW2, db2, dX, d eps)
and the add pooling, against the float64 restatement of torch_geometric.nn.GINConv (tests/gin_ref.py) at the project's bar —
|err| <= 1e-5 x the magnitude sum of the terms, and 1e-5 relative on the elements that are not cancellations (``_close`` of
test_gpu_gcn.py, over hops built by its ``_hop``: rows of degree 0, sampled loops, duplicates, hub sources)."""
import pytest

from gcn_ref import propagate
from gin_ref import gin_aggregate, gin_forward, mlp
from test_gpu_gcn import _close, _edge_index, _hop

pytestmark = pytest.mark.gpu

SHAPES = [(100, 256, 256), (128, 128, 128), (256, 256, 47), (64, 16, 16), (4, 4, 1)]
OUTSIDE = (300, 64, 64)


def _mlp_conv(F, H, N, seed, **kw):
    import torch
    from wholegraph_amd import nn
    torch.manual_seed(seed)
    return nn.GINConv(torch.nn.Sequential(torch.nn.Linear(F, H), torch.nn.ReLU(), torch.nn.Linear(H, N)), **kw).cuda()


def _params(conv):
    return [p.detach() for p in (conv.nn[0].weight, conv.nn[0].bias, conv.nn[2].weight, conv.nn[2].bias)]


def _layer_graph(rp, col, self_rows):
    from wholegraph_amd import nn
    return nn.LayerGraph([nn.HopGraph(rp, col, self_rows)])


@pytest.fixture
def launches(monkeypatch):
    """Counts the one-kernel launches (``gin_layer_forward`` calls) of the test."""
    import wholegraph_amd.nn as wnn
    calls, orig = [], wnn.gin_layer_forward

    def counted(*a, **kw):
        calls.append(1)
        return orig(*a, **kw)
    monkeypatch.setattr(wnn, "gin_layer_forward", counted)
    return calls


@pytest.mark.parametrize("F,H,N", SHAPES + [OUTSIDE])
@pytest.mark.parametrize("ids", [None, "int32", "int64"])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.3])
def test_layer_forward_vs_fp64(hiplib, launches, F, H, N, ids, relu, eps):
    """The layer over a hop with rows of degree 0, sampled loops (summed like any edge), duplicates and hub sources, x a tensor
    or read through a node list (LazyRows, int32 / int64 ids): ONE launch inside the kernel's domain, none outside it
    (F = 300: aggregate kernel, then nn)."""
    import torch
    from wholegraph_amd import nn
    n_src, n_dst = 3000, 1700
    rp, col, self_rows = _hop(n_dst, n_src, 24, seed=F + H + N)
    table = torch.randn((5000, F), device="cuda")
    if ids is None:
        x, xd = table[:n_src].contiguous(), table[:n_src]
    else:
        idv = torch.randperm(5000, device="cuda")[:n_src].to(getattr(torch, ids))
        x, xd = nn.LazyRows(table, idv), table[idv.long()]
    conv = _mlp_conv(F, H, N, seed=1, eps=eps)
    with torch.no_grad():
        got = conv(x, _layer_graph(rp, col, self_rows), act="relu" if relu else None)
    assert conv.route == ("aggregate" if (F, H, N) == OUTSIDE else "mlp")
    assert len(launches) == (0 if (F, H, N) == OUTSIDE else 1)
    ei = _edge_index(rp, col, self_rows)
    ref = gin_forward(xd, ei, *_params(conv), eps=eps, relu=relu)[self_rows]
    scale = gin_forward(xd, ei, *_params(conv), eps=eps, abs_terms=True)[self_rows]
    assert got.shape == (n_dst, N)
    _close(got, ref, scale, "forward")


@pytest.mark.parametrize("form", ["linear", "linear_relu", "linear_relu_act", "mlp_tail", "batchnorm", "odd_hidden", "identity"])
def test_other_routes_vs_fp64(hiplib, launches, form):
    """The one-product kernel (an nn that starts with a Linear; the rest runs as it is) and the aggregate-only kernel."""
    import torch
    from wholegraph_amd import nn
    T = torch.nn
    F, H, N = 64, 32, 8
    n_src, n_dst = 2000, 1200
    rp, col, self_rows = _hop(n_dst, n_src, 16, seed=11)
    x = torch.randn((n_src, F), device="cuda")
    ei = _edge_index(rp, col, self_rows)
    torch.manual_seed(3)
    net, act = {
        "linear": (T.Linear(F, H), None),
        "linear_relu": (T.Sequential(T.Linear(F, H), T.ReLU()), None),
        "linear_relu_act": (T.Linear(F, H), "relu"),
        "mlp_tail": (T.Sequential(T.Linear(F, H), T.ReLU(), T.Linear(H, N), T.ReLU()), None),
        "batchnorm": (T.Sequential(T.Linear(F, H), T.BatchNorm1d(H), T.ReLU(), T.Linear(H, N)), None),
        "odd_hidden": (T.Sequential(T.Linear(F, 30), T.ReLU(), T.Linear(30, N)), "relu"),
        "identity": (T.Identity(), None),
    }[form]
    conv = nn.GINConv(net, eps=0.2).cuda()
    with torch.no_grad():
        got = conv(x, _layer_graph(rp, col, self_rows), act=act)
    assert conv.route == ("aggregate" if form == "identity" else "linear")
    assert len(launches) == (0 if form == "identity" else 1)
    agg = gin_aggregate(x, ei, 0.2)[self_rows]
    agg_abs = gin_aggregate(x, ei, 0.2, abs_terms=True)[self_rows]
    if form == "identity":
        ref, scale = agg, agg_abs
    elif form in ("linear", "linear_relu", "linear_relu_act"):
        lin = net if isinstance(net, T.Linear) else net[0]
        ref = mlp(agg, lin.weight.detach(), lin.bias.detach(), relu_hidden=form != "linear")
        scale = mlp(agg_abs, lin.weight.detach(), lin.bias.detach(), abs_terms=True)
    elif form == "batchnorm":
        # training-mode statistics over all rows, in float64
        w1, b1, w2, b2 = (p.detach().double() for p in (net[0].weight, net[0].bias, net[3].weight, net[3].bias))
        z = agg @ w1.t() + b1
        z_abs = agg_abs @ w1.abs().t() + b1.abs()
        mean, var = z.mean(0), z.var(0, unbiased=False)
        inv = (var + net[1].eps).rsqrt()
        ref = torch.relu((z - mean) * inv) @ w2.t() + b2
        scale = ((z_abs + mean.abs()) * inv) @ w2.abs().t() + b2.abs()
    else:
        lin1, lin2 = net[0], net[2]
        ref = mlp(agg, lin1.weight.detach(), lin1.bias.detach(), lin2.weight.detach(), lin2.bias.detach(), relu=True)
        scale = mlp(agg_abs, lin1.weight.detach(), lin1.bias.detach(), lin2.weight.detach(), lin2.bias.detach(), abs_terms=True)
    _close(got, ref, scale, form)


def test_graph_forms_give_the_same_rows(hiplib):
    """A COO edge_index with loops and duplicates, the [row_ptr, col] CSR pair of the same edges and a LayerGraph over them."""
    import torch
    from wholegraph_amd import nn
    n, F, H, N = 2500, 100, 64, 47
    g = torch.Generator(device="cuda").manual_seed(7)
    E = 30000
    ei = torch.stack([torch.randint(0, n, (E,), generator=g, device="cuda"), torch.randint(0, n - 50, (E,), generator=g, device="cuda")])
    ei[1, :300] = ei[0, :300]                      # self loops
    ei = torch.cat([ei, ei[:, 1000:1500]], 1)      # duplicate edges
    conv = _mlp_conv(F, H, N, seed=4, eps=-0.1)
    x = torch.randn((n, F), device="cuda")
    with torch.no_grad():
        got = conv(x, ei, act="relu")
    ref = gin_forward(x, ei, *_params(conv), eps=-0.1, relu=True)
    scale = gin_forward(x, ei, *_params(conv), eps=-0.1, abs_terms=True)
    assert got.shape == (n, N)
    _close(got, ref, scale, "edge_index")
    order = torch.sort(ei[1], stable=True).indices
    rp = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    rp[1:] = torch.cumsum(torch.bincount(ei[1], minlength=n), 0)
    col = ei[0][order].to(torch.int32).contiguous()
    with torch.no_grad():
        got2 = conv(x, [rp, col], act="relu")
        got3 = conv(x, nn.LayerGraph([nn.HopGraph(rp, col, torch.arange(n, device="cuda"))]), act="relu")
    assert torch.equal(got, got2) and torch.equal(got, got3)
    # a CSR pair over fewer destinations: the first rows of x
    with torch.no_grad():
        got4 = conv(x, [rp[:1001].contiguous(), col[:int(rp[1000])].contiguous()], act="relu")
    assert torch.equal(got4, got[:1000])
    # gradients through the edge_index path against float64 autograd
    xg = x.clone().requires_grad_(True)
    conv(xg, ei).sum().backward()
    xr = x.double().requires_grad_(True)
    gin_forward(xr, ei, *_params(conv), eps=-0.1).sum().backward()
    assert float((xg.grad.double() - xr.grad).abs().max()) <= 1e-5 * max(1.0, float(xr.grad.abs().max()))


@pytest.mark.parametrize("F,H,N", [(64, 32, 16), OUTSIDE])
def test_bipartite_pair(hiplib, F, H, N):
    """(x_src, x_dst) with more destinations than sources, and (x_src, None): no root term."""
    import torch
    n_src, n_dst, E = 500, 900, 6000
    g = torch.Generator(device="cuda").manual_seed(F)
    ei = torch.stack([torch.randint(0, n_src, (E,), generator=g, device="cuda"), torch.randint(0, n_dst, (E,), generator=g, device="cuda")])
    ei[1, 0] = n_dst - 1
    conv = _mlp_conv(F, H, N, seed=5, eps=0.4, train_eps=True)
    xs, xt = torch.randn((n_src, F), device="cuda"), torch.randn((n_dst, F), device="cuda")
    p = _params(conv)
    with torch.no_grad():
        got = conv((xs, xt), ei)
        got_none = conv((xs, None), ei, act="relu")
    assert got.shape == (n_dst, N) and got_none.shape == (n_dst, N)
    _close(got, gin_forward(xs, ei, *p, eps=0.4, x_dst=xt), gin_forward(xs, ei, *p, eps=0.4, x_dst=xt, abs_terms=True), "pair")
    _close(got_none, gin_forward(xs, ei, *p, eps=0.4, root=False, relu=True), gin_forward(xs, ei, *p, root=False, abs_terms=True),
           "no root")
    # gradients of both inputs and of eps against float64 autograd
    a, b = xs.clone().requires_grad_(True), xt.clone().requires_grad_(True)
    R = torch.randn((n_dst, N), device="cuda")
    (conv((a, b), ei) * R).sum().backward()
    a64, b64 = xs.double().requires_grad_(True), xt.double().requires_grad_(True)
    e64 = torch.tensor(0.4, dtype=torch.float64, device="cuda", requires_grad=True)
    agg = torch.zeros((n_dst, F), dtype=torch.float64, device="cuda").index_add_(0, ei[1], a64[ei[0]]) + (1 + e64) * b64
    (mlp(agg, *p) * R.double()).sum().backward()
    for got_g, want, what in ((a.grad, a64.grad, "dx_src"), (b.grad, b64.grad, "dx_dst"), (conv.eps.grad, e64.grad.reshape(1), "d eps")):
        assert float((got_g.double() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max())), what
    # (x_src, None): eps has no part in the output
    conv.zero_grad(set_to_none=True)
    a = xs.clone().requires_grad_(True)
    (conv((a, None), ei) * R).sum().backward()
    a64 = xs.double().requires_grad_(True)
    (gin_forward(a64, ei, *p, root=False) * R.double()).sum().backward()
    assert float((a.grad.double() - a64.grad).abs().max()) <= 1e-5 * max(1.0, float(a64.grad.abs().max()))
    assert conv.eps.grad is None or float(conv.eps.grad.abs().max()) == 0.0


@pytest.mark.parametrize("F,H,N", SHAPES + [OUTSIDE])
@pytest.mark.parametrize("relu", [False, True])
def test_layer_backward_vs_fp64_and_deterministic(hiplib, F, H, N, relu):
    """dW1, db1, dW2, db2, dX and d eps against float64 with their own magnitude sums, the ReLU masks taken from the activations
    the layer itself stored (output and hidden); two backward passes bit for bit the same."""
    import torch
    from wholegraph_amd import nn
    n_src, n_dst, eps = 2600, 1500, 0.3
    rp, col, self_rows = _hop(n_dst, n_src, 20, seed=3 * F + H + N)
    conv = _mlp_conv(F, H, N, seed=2, eps=eps, train_eps=True)
    x0 = torch.randn((n_src, F), device="cuda")
    R = torch.randn((n_dst, N), device="cuda")
    lg = _layer_graph(rp, col, self_rows)
    grads = []
    for _ in range(2):
        conv.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        out = conv(x, lg, act="relu" if relu else None)
        (out * R).sum().backward()
        grads.append([conv.nn[0].weight.grad.clone(), conv.nn[0].bias.grad.clone(), conv.nn[2].weight.grad.clone(),
                      conv.nn[2].bias.grad.clone(), x.grad.clone(), conv.eps.grad.clone(), out.detach().clone()])
    for a, b in zip(grads[0], grads[1]):
        assert torch.equal(a, b), "backward is not run-to-run deterministic"
    gw1, gb1, gw2, gb2, gx, geps, out = grads[0]
    W1, b1, W2, b2 = (p.double() for p in _params(conv))
    # the hidden activation as the layer stored it
    with torch.no_grad():
        if (F, H, N) == OUTSIDE:
            hidden = conv.nn[1](conv.nn[0](nn.gin_aggregate(rp, col, x0, self_rows, eps=conv.eps.detach())))
        else:
            out_k, agg_k, hidden = nn.gin_layer_forward(rp, col, x0, self_rows, *_params(conv), eps=conv.eps.detach(), relu_out=relu,
                                                        keep=True)
            assert torch.equal(out_k, out)
            _close(agg_k, gin_aggregate(x0, _edge_index(rp, col, self_rows), eps)[self_rows],
                   gin_aggregate(x0, _edge_index(rp, col, self_rows), eps, abs_terms=True)[self_rows], "stored aggregate")
    ei = _edge_index(rp, col, self_rows)
    agg = gin_aggregate(x0, ei, eps)[self_rows]
    agg_abs = gin_aggregate(x0, ei, eps, abs_terms=True)[self_rows]
    hmask = (hidden > 0).double()
    hid = (agg @ W1.t() + b1) * hmask
    hid_abs = (agg_abs @ W1.abs().t() + b1.abs()) * hmask
    dz2 = R.double() * ((out > 0).double() if relu else 1.0)
    _close(gw2, dz2.t() @ hid, dz2.abs().t() @ hid_abs, "dW2")
    _close(gb2, dz2.sum(0), dz2.abs().sum(0), "db2")
    g1, g1_abs = (dz2 @ W2) * hmask, (dz2.abs() @ W2.abs()) * hmask
    _close(gw1, g1.t() @ agg, g1_abs.t() @ agg_abs, "dW1")
    _close(gb1, g1.sum(0), g1_abs.sum(0), "db1")
    full = torch.zeros((n_src, F), dtype=torch.float64, device="cuda")
    full_abs = torch.zeros_like(full)
    full[self_rows], full_abs[self_rows] = g1 @ W1, g1_abs @ W1.abs()
    one = torch.ones(ei.shape[1], dtype=torch.float64)
    # dX = A^T dAgg + (1 + eps) dAgg at the rows that are destinations
    _close(gx, propagate(ei[1], ei[0], one, full) + (1 + eps) * full, propagate(ei[1], ei[0], one, full_abs) + (1 + eps) * full_abs, "dX")
    xs = x0.double()[self_rows]
    _close(geps, (full[self_rows] * xs).sum().reshape(1), (full_abs[self_rows] * xs.abs()).sum().reshape(1), "d eps")


@pytest.mark.parametrize("relu", [False, True])
def test_one_product_backward_vs_fp64(hiplib, relu):
    """The nn = Sequential(Linear, ReLU) route: its output is the activation the mask is taken from."""
    import torch
    from wholegraph_amd import nn
    F, H, n_src, n_dst, eps = 100, 47, 2000, 1100, -0.2
    rp, col, self_rows = _hop(n_dst, n_src, 20, seed=9)
    torch.manual_seed(6)
    net = torch.nn.Sequential(torch.nn.Linear(F, H), torch.nn.ReLU()) if relu else torch.nn.Linear(F, H)
    conv = nn.GINConv(net, eps=eps, train_eps=True).cuda()
    lin = net[0] if relu else net
    x0 = torch.randn((n_src, F), device="cuda")
    R = torch.randn((n_dst, H), device="cuda")
    x = x0.clone().requires_grad_(True)
    out = conv(x, _layer_graph(rp, col, self_rows))
    (out * R).sum().backward()
    ei = _edge_index(rp, col, self_rows)
    W1 = lin.weight.detach().double()
    agg = gin_aggregate(x0, ei, eps)[self_rows]
    agg_abs = gin_aggregate(x0, ei, eps, abs_terms=True)[self_rows]
    g1 = R.double() * ((out > 0).double() if relu else 1.0)
    _close(lin.weight.grad, g1.t() @ agg, g1.abs().t() @ agg_abs, "dW1")
    _close(lin.bias.grad, g1.sum(0), g1.abs().sum(0), "db1")
    full = torch.zeros((n_src, F), dtype=torch.float64, device="cuda")
    full_abs = torch.zeros_like(full)
    full[self_rows], full_abs[self_rows] = g1 @ W1, g1.abs() @ W1.abs()
    one = torch.ones(ei.shape[1], dtype=torch.float64)
    _close(x.grad, propagate(ei[1], ei[0], one, full) + (1 + eps) * full, propagate(ei[1], ei[0], one, full_abs) + (1 + eps) * full_abs,
           "dX")
    xs = x0.double()[self_rows]
    _close(conv.eps.grad, (full[self_rows] * xs).sum().reshape(1), (full_abs[self_rows] * xs.abs()).sum().reshape(1), "d eps")


@pytest.mark.parametrize("F,H,N", [(32, 24, 8), OUTSIDE])
def test_layer_graph_with_an_edgeless_hop(hiplib, F, H, N):
    """Two hops, the second without edges: its rows are nn((1 + eps) x_self); forward and backward against float64 autograd."""
    import torch
    from wholegraph_amd import nn
    n_src = 300
    g = torch.Generator(device="cuda").manual_seed(3)
    deg = torch.randint(0, 7, (80,), generator=g, device="cuda")
    rp0 = torch.zeros(81, dtype=torch.int32, device="cuda")
    rp0[1:] = torch.cumsum(deg, 0)
    col0 = torch.randint(0, n_src, (int(rp0[-1]),), generator=g, device="cuda", dtype=torch.int32)
    perm = torch.randperm(n_src, generator=g, device="cuda")
    h0 = nn.HopGraph(rp0, col0, perm[:80].contiguous())
    h1 = nn.HopGraph(torch.zeros(41, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"),
                     perm[80:120].contiguous())
    lg = nn.LayerGraph([h0, h1])
    ei = torch.stack([col0.long(), h0.self_rows[torch.repeat_interleave(torch.arange(80, device="cuda"), deg)]])
    dst = torch.cat([h0.self_rows, h1.self_rows])
    conv = _mlp_conv(F, H, N, seed=8, eps=0.1, train_eps=True)
    x = torch.randn((n_src, F), generator=g, device="cuda")
    xg = x.clone().requires_grad_(True)
    out = conv(xg, lg, act="relu")
    R = torch.randn(out.shape, generator=g, device="cuda")
    (out * R).sum().backward()
    xr = x.double().requires_grad_(True)
    p64 = [p.double().requires_grad_(True) for p in _params(conv)]
    e64 = torch.tensor(0.1, dtype=torch.float64, device="cuda", requires_grad=True)
    agg = torch.zeros((n_src, F), dtype=torch.float64, device="cuda").index_add_(0, ei[1], xr[ei[0]]) + (1 + e64) * xr
    pre = torch.relu(agg[dst] @ p64[0].t() + p64[1]) @ p64[2].t() + p64[3]
    ref = pre * (out.detach() > 0).double()
    (ref * R.double()).sum().backward()
    assert out.shape == (120, N)
    scale = gin_forward(x, ei, *_params(conv), eps=0.1, abs_terms=True)[dst]
    _close(out.detach(), ref.detach(), scale, "edgeless hop forward")
    got = [xg.grad, conv.nn[0].weight.grad, conv.nn[0].bias.grad, conv.nn[2].weight.grad, conv.nn[2].bias.grad, conv.eps.grad]
    want = [xr.grad] + [p.grad for p in p64] + [e64.grad.reshape(1)]
    for a, b, what in zip(got, want, ("dX", "dW1", "db1", "dW2", "db2", "d eps")):
        assert float((a.double() - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max())), what
    # a layer graph without any row
    empty = nn.LayerGraph([nn.HopGraph(torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"),
                                       torch.zeros(0, dtype=torch.int64, device="cuda"))])
    xg = x.clone().requires_grad_(True)
    out = conv(xg, empty)
    assert out.shape == (0, N)
    out.sum().backward()
    assert float(xg.grad.abs().max()) == 0.0


def test_refusals(hiplib):
    import torch
    import wholegraph_amd.nn as wnn
    rp, col, self_rows = _hop(100, 300, 5, seed=1)
    conv = _mlp_conv(16, 8, 8, seed=0)
    lg = _layer_graph(rp, col, self_rows)
    table = torch.randn(500, 16, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError):
        conv(wnn.LazyRows(table, torch.arange(300, device="cuda")), lg)
    with pytest.raises(NotImplementedError):
        conv((torch.randn(300, 16, device="cuda"), torch.randn(100, 16, device="cuda")), lg)
    with pytest.raises(ValueError):
        conv(None, lg)
    orig = wnn._capturing
    wnn._capturing = lambda: True
    try:
        with pytest.raises(RuntimeError, match="capture"):
            conv(torch.randn(300, 16, device="cuda"), lg)
    finally:
        wnn._capturing = orig


@pytest.mark.parametrize("F", [1, 47, 64, 200])
def test_global_add_pool(hiplib, F):
    """A sorted batch (bitwise repeatable, against float64) with empty graphs in the middle and past batch.max(), ``ptr``, the
    unsorted fallback and the gradient."""
    import torch
    from wholegraph_amd.nn import global_add_pool
    g = torch.Generator(device="cuda").manual_seed(F)
    G = 300
    counts = torch.randint(0, 40, (G,), generator=g, device="cuda")
    counts[[3, 4, 150]] = 0                                   # empty graphs in the middle
    counts[7] = 900                                           # one long segment
    batch = torch.repeat_interleave(torch.arange(G, device="cuda"), counts)
    n = batch.shape[0]
    x = torch.randn((n, F), generator=g, device="cuda")
    size = G + 5                                              # larger than batch.max() + 1
    ref = torch.zeros((size, F), dtype=torch.float64, device="cuda").index_add_(0, batch, x.double())
    scale = torch.zeros((size, F), dtype=torch.float64, device="cuda").index_add_(0, batch, x.double().abs())
    got = global_add_pool(x, batch, size=size)
    assert got.shape == (size, F)
    assert torch.equal(got, global_add_pool(x, batch, size=size)), "not bitwise repeatable"
    _close(got, ref, scale, "sorted")
    assert float(got[[3, 4, 150]].abs().max()) == 0.0 and float(got[G:].abs().max()) == 0.0
    assert torch.equal(global_add_pool(x, batch)[:G], got[:int(batch.max()) + 1][:G])
    ptr = torch.zeros(G + 1, dtype=torch.int64, device="cuda")
    ptr[1:] = torch.cumsum(counts, 0)
    assert torch.equal(global_add_pool(x, batch, ptr=ptr), got[:G])
    # a view with a row stride
    wide = torch.randn((n, F + 3), generator=g, device="cuda")
    _close(global_add_pool(wide[:, :F], batch, size=size),
           torch.zeros((size, F), dtype=torch.float64, device="cuda").index_add_(0, batch, wide[:, :F].double()),
           torch.zeros((size, F), dtype=torch.float64, device="cuda").index_add_(0, batch, wide[:, :F].double().abs()), "strided")
    # unsorted: index_add_
    perm = torch.randperm(n, generator=g, device="cuda")
    _close(global_add_pool(x[perm], batch[perm], size=size), ref, scale, "unsorted")
    # gradient: grad[batch], on both routes
    R = torch.randn((size, F), generator=g, device="cuda")
    for xs, bs in ((x, batch), (x[perm], batch[perm])):
        xg = xs.clone().requires_grad_(True)
        (global_add_pool(xg, bs, size=size) * R).sum().backward()
        assert torch.equal(xg.grad, R[bs])
