"""GPU parity of the batch-norm route of wholegraph_amd.nn.GINConv — ``GINConv(nn.MLP([F, H, N]))``, route "mlp_bn"
(csrc/wg_gin.hip's STATS variant and csrc/wg_batch_norm.hip): the training forward (layer kernel with per-tile statistics,
finalize, fused tail) with its running statistics, the eval forward on the folded weights, layer graphs whose hops end in
partial tiles, every gradient (dW1, db1, dgamma, dbeta, dW2, db2, dX, d eps), the column statistics on their own at a mean far
from zero, and the graph forms — against float64 torch (``torch.nn.BatchNorm1d`` written out; tests/gin_ref.py for the aggregate)
at the project's bar: |err| <= 1e-5 x the magnitude sum of the terms + 1e-7, and 1e-5 relative where the result is no
cancellation (``_close`` of test_gpu_gcn.py).  A magnitude sum is the reference formula with the absolute values of its terms and
every subtraction turned into an addition."""
import pytest

from gcn_ref import propagate
from gin_ref import gin_aggregate
from test_gpu_gcn import _close, _edge_index, _hop

pytestmark = pytest.mark.gpu

SHAPES = [(64, 32, 8), (100, 256, 256), (4, 4, 1), (256, 256, 47)]
N_DST = 1500


def _bn_conv(F, H, N, seed, **kw):
    """GINConv(MLP([F, H, N])) on the device, gamma and beta away from (1, 0)."""
    import torch
    from wholegraph_amd import nn
    torch.manual_seed(seed)
    conv = nn.GINConv(nn.MLP([F, H, N]), **kw)
    bn = conv.nn.norms[0].module
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
    return conv.cuda()


def _parts(conv):
    return conv.nn.lins[0], conv.nn.norms[0].module, conv.nn.lins[1]


class _Ref:
    """The layer behind the aggregate in float64 with the magnitude sum of every stage (``*_abs``).  ``stats``: (mean, var) to
    normalise with (eval mode: the running statistics); None: the batch's own, with the assertion that no column's variance
    is small enough for rstd to amplify anything."""

    def __init__(self, conv, agg, agg_abs, relu=False, stats=None):
        import torch
        lin1, bn, lin2 = _parts(conv)
        d = lambda t: t.detach().double()      # noqa: E731
        self.W1, self.b1, self.W2, self.b2, self.gamma, self.beta = (d(t) for t in (lin1.weight, lin1.bias, lin2.weight, lin2.bias,
                                                                                      bn.weight, bn.bias))
        self.n = agg.shape[0]
        self.agg, self.agg_abs = agg, agg_abs
        self.z = agg @ self.W1.t() + self.b1
        self.z_abs = agg_abs @ self.W1.abs().t() + self.b1.abs()
        if stats is None:
            self.mean, self.var = self.z.mean(0), self.z.var(0, unbiased=False)
            assert float(self.var.min()) >= 0.1, "a column variance near zero: rstd would amplify the rounding of z"
        else:
            self.mean, self.var = (d(t) for t in stats)
        self.rstd = (self.var + bn.eps).rsqrt()
        self.xhat = (self.z - self.mean) * self.rstd
        self.xhat_abs = (self.z_abs + self.mean.abs()) * self.rstd
        self.y = self.xhat * self.gamma + self.beta
        self.y_abs = self.xhat_abs * self.gamma.abs() + self.beta.abs()
        out = torch.relu(self.y) @ self.W2.t() + self.b2
        self.out = torch.relu(out) if relu else out
        self.out_abs = self.y_abs @ self.W2.abs().t() + self.b2.abs()
        # what one training step leaves in the running statistics (momentum m, from the initial 0 and 1)
        m = bn.momentum
        self.run_mean, self.run_mean_abs = m * self.mean, m * self.z_abs.mean(0)
        if self.n > 1:
            self.run_var = (1 - m) + m * self.z.var(0, unbiased=True)
            self.run_var_abs = (1 - m) + m * ((self.z_abs + self.mean.abs()) ** 2).sum(0) / (self.n - 1)


def _hop_ref(conv, xd, rp, col, self_rows, eps, relu=False, stats=None):
    ei = _edge_index(rp, col, self_rows)
    return _Ref(conv, gin_aggregate(xd, ei, eps)[self_rows], gin_aggregate(xd, ei, eps, abs_terms=True)[self_rows], relu, stats)


def _layer_graph(*hops):
    from wholegraph_amd import nn
    return nn.LayerGraph([nn.HopGraph(*h) for h in hops])


@pytest.fixture
def launches(monkeypatch):
    """Counts the calls of the launch wrappers: the "mlp" kernel, and the batch-norm route's three."""
    import wholegraph_amd.nn as wnn
    calls = {}

    def count(name):
        orig = getattr(wnn, name)
        calls[name] = 0

        def counted(*a, **kw):
            calls[name] += 1
            return orig(*a, **kw)
        monkeypatch.setattr(wnn, name, counted)
    for name in ("gin_layer_forward", "gin_layer_stats", "bn_finalize", "bn_act_linear"):
        count(name)
    return calls


@pytest.mark.parametrize("F,H,N", SHAPES)
@pytest.mark.parametrize("ids", [None, "int32", "int64"])
@pytest.mark.parametrize("relu", [False, True])
def test_training_forward_vs_fp64(hiplib, launches, F, H, N, ids, relu):
    """One training step: the output, the running statistics it leaves and the launches it takes — the stats kernel once per hop,
    the finalize and the tail once per layer, the "mlp" kernel never."""
    import torch
    from wholegraph_amd import nn
    n_src, eps = 2600, 0.3
    rp, col, self_rows = _hop(N_DST, n_src, 20, seed=F + H + N)
    table = torch.randn((4000, F), device="cuda")
    if ids is None:
        x, xd = table[:n_src].contiguous(), table[:n_src]
    else:
        idv = torch.randperm(4000, device="cuda")[:n_src].to(getattr(torch, ids))
        x, xd = nn.LazyRows(table, idv), table[idv.long()]
    conv = _bn_conv(F, H, N, seed=1, eps=eps)
    assert conv.route == "mlp_bn" and conv.training
    with torch.no_grad():
        got = conv(x, _layer_graph((rp, col, self_rows)), act="relu" if relu else None)
    assert launches == {"gin_layer_forward": 0, "gin_layer_stats": 1, "bn_finalize": 1, "bn_act_linear": 1}
    ref = _hop_ref(conv, xd, rp, col, self_rows, eps, relu)
    assert got.shape == (N_DST, N)
    _close(got, ref.out, ref.out_abs, "forward")
    bn = _parts(conv)[1]
    _close(bn.running_mean, ref.run_mean, ref.run_mean_abs, "running_mean")
    _close(bn.running_var, ref.run_var, ref.run_var_abs, "running_var")
    assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("F,H,N", SHAPES)
@pytest.mark.parametrize("relu", [False, True])
def test_eval_forward_vs_fp64(hiplib, launches, F, H, N, relu):
    """Eval mode after two training steps: the running statistics fold into W1, b1 — exactly one "mlp" kernel launch per hop,
    none of the batch-norm launches, the running buffers untouched; and the fold is made once per weight change."""
    import torch
    import wholegraph_amd.nn as wnn
    n_src, eps = 2600, -0.2
    rp, col, self_rows = _hop(N_DST, n_src, 20, seed=2 * F + H + N)
    lg = _layer_graph((rp, col, self_rows))
    x = torch.randn((n_src, F), device="cuda")
    conv = _bn_conv(F, H, N, seed=3, eps=eps)
    with torch.no_grad():
        conv(x, lg)
        conv(0.5 * x + 0.25, lg)
    lin1, bn, lin2 = _parts(conv)
    assert int(bn.num_batches_tracked) == 2
    before = [t.clone() for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]
    for k in launches:
        launches[k] = 0
    conv.eval()
    with torch.no_grad():
        got = conv(x, lg, act="relu" if relu else None)
        folded = wnn._bn_folded_linear(lin1, bn, False)
        again = conv(x, lg, act="relu" if relu else None)
    assert launches == {"gin_layer_forward": 2, "gin_layer_stats": 0, "bn_finalize": 0, "bn_act_linear": 0}
    assert wnn._bn_folded_linear(lin1, bn, False)[0] is folded[0] and torch.equal(got, again)
    for a, b in zip(before, (bn.running_mean, bn.running_var, bn.num_batches_tracked)):
        assert torch.equal(a, b)
    ref = _hop_ref(conv, x, rp, col, self_rows, eps, relu, stats=(bn.running_mean, bn.running_var))
    _close(got, ref.out, ref.out_abs, "eval forward")
    # a weight change makes a new fold
    with torch.no_grad():
        bn.weight.mul_(2.0)
        got2 = conv(x, lg, act="relu" if relu else None)
    ref2 = _hop_ref(conv, x, rp, col, self_rows, eps, relu, stats=(bn.running_mean, bn.running_var))
    _close(got2, ref2.out, ref2.out_abs, "eval forward after a weight change")


def test_eval_gradients_flow_through_the_fold(hiplib):
    """Parameters that require grad in eval mode: the fold is autograd-visible, every parameter gets its gradient."""
    import torch
    F, H, N, n_src = 64, 32, 8, 900
    rp, col, self_rows = _hop(500, n_src, 12, seed=5)
    lg = _layer_graph((rp, col, self_rows))
    x = torch.randn((n_src, F), device="cuda")
    conv = _bn_conv(F, H, N, seed=4, eps=0.1)
    with torch.no_grad():
        conv(x, lg)
    conv.eval()
    lin1, bn, lin2 = _parts(conv)
    R = torch.randn((500, N), device="cuda")
    xg = x.clone().requires_grad_(True)
    (conv(xg, lg) * R).sum().backward()
    p64 = [t.detach().double().requires_grad_(True) for t in (lin1.weight, lin1.bias, bn.weight, bn.bias, lin2.weight, lin2.bias)]
    x64 = x.double().requires_grad_(True)
    ei = _edge_index(rp, col, self_rows)
    agg = (torch.zeros((n_src, F), dtype=torch.float64, device="cuda").index_add_(0, ei[1], x64[ei[0]]) + 1.1 * x64)[self_rows]
    y = (agg @ p64[0].t() + p64[1] - bn.running_mean.double()) * (bn.running_var.double() + bn.eps).rsqrt() * p64[2] + p64[3]
    ((torch.relu(y) @ p64[4].t() + p64[5]) * R.double()).sum().backward()
    got = [lin1.weight.grad, lin1.bias.grad, bn.weight.grad, bn.bias.grad, lin2.weight.grad, lin2.bias.grad, xg.grad]
    for a, b, what in zip(got, [p.grad for p in p64] + [x64.grad], ("dW1", "db1", "dgamma", "dbeta", "dW2", "db2", "dX")):
        assert a is not None, what
        assert float((a.double() - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max())), what


def _small_hop(n_rows, n_src, g, max_deg=6):
    import torch
    deg = torch.randint(0, max_deg + 1, (n_rows,), generator=g, device="cuda") if max_deg > 0 else torch.zeros(n_rows, dtype=torch.long, device="cuda")
    rp = torch.zeros(n_rows + 1, dtype=torch.int32, device="cuda")
    rp[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, n_src, (int(rp[-1]),), generator=g, device="cuda", dtype=torch.int32)
    self_rows = torch.randperm(n_src, generator=g, device="cuda")[:n_rows].contiguous()
    return rp, col, self_rows


@pytest.mark.parametrize("sizes", [(17, 20), (17, 20, 9), (1, 1)], ids=["two_partial_tiles", "with_an_edgeless_hop", "two_rows"])
def test_hops_with_partial_tiles(hiplib, launches, sizes):
    """A layer graph whose hops all end in a partial tile (17 and 20 rows): the tile counts carry the statistics; with an edgeless
    hop behind them; and 2 rows in all, the smallest legal batch."""
    import torch
    F, H, N, n_src, eps = 32, 24, 8, 120, 0.1
    g = torch.Generator(device="cuda").manual_seed(sum(sizes))
    hops = [_small_hop(n, n_src, g, max_deg=0 if (len(sizes) == 3 and k == 2) else 6) for k, n in enumerate(sizes)]
    x = torch.randn((n_src, F), generator=g, device="cuda")
    conv = _bn_conv(F, H, N, seed=6, eps=eps)
    aggs = [(gin_aggregate(x, _edge_index(*h), eps)[h[2]], gin_aggregate(x, _edge_index(*h), eps, abs_terms=True)[h[2]]) for h in hops]
    if sizes == (1, 1):
        # two rows: W1 = c d^T / |d|^2 with d the difference of the two aggregates, so column h of z differs by c[h], 1 <= |c[h]| < 2,
        # between them and every variance is c[h]^2 / 4 >= 0.25
        d = (aggs[0][0] - aggs[1][0])[0]
        c = (1.0 + torch.arange(H, dtype=torch.float64, device="cuda") / H) * (1.0 - 2.0 * (torch.arange(H, device="cuda") % 2))
        with torch.no_grad():
            _parts(conv)[0].weight.copy_((c[:, None] * d[None, :] / (d @ d)).float())
    with torch.no_grad():
        got = conv(x, _layer_graph(*hops), act="relu")
    assert launches == {"gin_layer_forward": 0, "gin_layer_stats": len(sizes), "bn_finalize": 1, "bn_act_linear": 1}
    ref = _Ref(conv, torch.cat([a for a, _ in aggs]), torch.cat([b for _, b in aggs]), relu=True)
    assert got.shape == (sum(sizes), N)
    _close(got, ref.out, ref.out_abs, "forward")
    bn = _parts(conv)[1]
    _close(bn.running_mean, ref.run_mean, ref.run_mean_abs, "running_mean")
    _close(bn.running_var, ref.run_var, ref.run_var_abs, "running_var")
    assert int(bn.num_batches_tracked) == 1


def test_one_row_is_refused_and_no_row_gives_no_row(hiplib):
    import torch
    F, H, N, n_src = 32, 24, 8, 50
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((n_src, F), generator=g, device="cuda")
    conv = _bn_conv(F, H, N, seed=7)
    bn = _parts(conv)[1]
    with pytest.raises(ValueError, match="more than 1"):
        conv(x, _layer_graph(_small_hop(1, n_src, g)))
    empty = _layer_graph((torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"),
                          torch.zeros(0, dtype=torch.int64, device="cuda")))
    xg = x.clone().requires_grad_(True)
    out = conv(xg, empty)
    assert out.shape == (0, N)
    out.sum().backward()
    assert float(xg.grad.abs().max()) == 0.0
    assert int(bn.num_batches_tracked) == 0 and float(bn.running_mean.abs().max()) == 0.0 and float((bn.running_var - 1).abs().max()) == 0.0
    conv.eval()
    assert conv(x, _layer_graph(_small_hop(1, n_src, g))).shape == (1, N)      # eval mode takes one row, as BatchNorm1d does


@pytest.mark.parametrize("F,H,N", SHAPES)
@pytest.mark.parametrize("relu", [False, True])
def test_backward_vs_fp64_and_deterministic(hiplib, F, H, N, relu):
    """dW1, db1, dgamma, dbeta, dW2, db2, dX and d eps against float64 with their own magnitude sums, the ReLU masks taken from
    the hidden activation and the output the layer itself stored; two runs bit for bit the same; a second backward refused."""
    import torch
    from wholegraph_amd import nn
    n_src, eps = 2600, 0.3
    rp, col, self_rows = _hop(N_DST, n_src, 20, seed=3 * F + H + N)
    conv = _bn_conv(F, H, N, seed=2, eps=eps, train_eps=True)
    lin1, bn, lin2 = _parts(conv)
    x0 = torch.randn((n_src, F), device="cuda")
    R = torch.randn((N_DST, N), device="cuda")
    lg = _layer_graph((rp, col, self_rows))
    params = (lin1.weight, lin1.bias, bn.weight, bn.bias, lin2.weight, lin2.bias, conv.eps)
    runs = []
    for _ in range(2):
        conv.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        out = conv(x, lg, act="relu" if relu else None)
        loss = (out * R).sum()
        loss.backward(retain_graph=True)
        runs.append([p.grad.clone() for p in params] + [x.grad.clone(), out.detach().clone()])
    with pytest.raises(RuntimeError):
        loss.backward()
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b), "backward is not run-to-run deterministic"
    gw1, gb1, ggamma, gbeta, gw2, gb2, geps, gx, out = runs[0]
    # what the layer stored: the same launches through the low-level entry, running statistics left alone
    with torch.no_grad():
        out_k, agg_k, z_k, hidden, mean_k, rstd_k = nn.gin_bn_forward(
            [(rp, col, self_rows, None)], x0, lin1.weight, lin1.bias, bn.weight, bn.bias, lin2.weight, lin2.bias, bn_eps=bn.eps,
            eps=conv.eps.detach(), relu_out=relu, keep=True)
    assert torch.equal(out_k, out)
    r = _hop_ref(conv, x0, rp, col, self_rows, eps, relu)
    _close(agg_k, r.agg, r.agg_abs, "stored aggregate")
    _close(z_k, r.z, r.z_abs, "stored z")
    _close(mean_k, r.mean, r.z_abs.mean(0), "mean")
    var_abs = ((r.z_abs + r.mean.abs()) ** 2).mean(0)          # d rstd = -rstd^3 d var / 2
    _close(rstd_k, r.rstd, r.rstd + 0.5 * r.rstd ** 3 * var_abs, "rstd")
    n = r.n
    hmask = (hidden > 0).double()
    hid, hid_abs = r.y * hmask, r.y_abs * hmask
    dz2 = R.double() * ((out > 0).double() if relu else 1.0)
    _close(gw2, dz2.t() @ hid, dz2.abs().t() @ hid_abs, "dW2")
    _close(gb2, dz2.sum(0), dz2.abs().sum(0), "db2")
    dy, dy_abs = (dz2 @ r.W2) * hmask, (dz2.abs() @ r.W2.abs()) * hmask
    dbeta, dbeta_abs = dy.sum(0), dy_abs.sum(0)
    dgamma, dgamma_abs = (dy * r.xhat).sum(0), (dy_abs * r.xhat_abs).sum(0)
    _close(gbeta, dbeta, dbeta_abs, "dbeta")
    _close(ggamma, dgamma, dgamma_abs, "dgamma")
    k = r.gamma * r.rstd
    dz = k * (dy - dbeta / n - r.xhat * dgamma / n)
    dz_abs = k.abs() * (dy_abs + dbeta_abs / n + r.xhat_abs * dgamma_abs / n)
    _close(gw1, dz.t() @ r.agg, dz_abs.t() @ r.agg_abs, "dW1")
    _close(gb1, dz.sum(0), dz_abs.sum(0), "db1")
    full = torch.zeros((n_src, F), dtype=torch.float64, device="cuda")
    full_abs = torch.zeros_like(full)
    full[self_rows], full_abs[self_rows] = dz @ r.W1, dz_abs @ r.W1.abs()
    ei = _edge_index(rp, col, self_rows)
    one = torch.ones(ei.shape[1], dtype=torch.float64)
    _close(gx, propagate(ei[1], ei[0], one, full) + (1 + eps) * full, propagate(ei[1], ei[0], one, full_abs) + (1 + eps) * full_abs, "dX")
    xs = x0.double()[self_rows]
    _close(geps, (full[self_rows] * xs).sum().reshape(1), (full_abs[self_rows] * xs.abs()).sum().reshape(1), "d eps")


def test_column_statistics_far_from_zero(hiplib):
    """z = 100 + 2 randn, [4099, 36] (a partial last tile, a width that is no power of two): mean and biased variance within 1e-5
    relative of the float64 statistics of the same float32 values.  The per-tile two-pass records combined with the pairwise
    update give 4.7e-7 and 9.8e-7 here in a float32 emulation; a one-pass sum and sum of squares gives 1.1e-2 on the variance."""
    import torch
    from wholegraph_amd import nn
    g = torch.Generator(device="cuda").manual_seed(0)
    z = 100.0 + 2.0 * torch.randn((4099, 36), generator=g, device="cuda")
    mean, var = nn.bn_column_stats(z)
    mean2, var2 = nn.bn_column_stats(z)
    assert torch.equal(mean, mean2) and torch.equal(var, var2), "not bitwise repeatable"
    m64, v64 = z.double().mean(0), z.double().var(0, unbiased=False)
    e_mean = float(((mean.double() - m64).abs() / m64.abs()).max())
    e_var = float(((var.double() - v64).abs() / v64).max())
    print("relative error: mean %.3g, variance %.3g" % (e_mean, e_var))
    assert mean.shape == (36,) and var.shape == (36,)
    assert e_mean <= 1e-5, e_mean
    assert e_var <= 1e-5, e_var
    # rows of a wider buffer (a leading dimension larger than the width)
    wide = torch.zeros((4099, 40), device="cuda")
    wide[:, :36] = z
    m3, v3 = nn.bn_column_stats(wide[:, :36])
    assert torch.equal(m3, mean) and torch.equal(v3, var)


def test_graph_forms_give_the_same_rows(hiplib):
    """A COO edge_index with loops and duplicates, the [row_ptr, col] CSR pair of the same edges and a LayerGraph over them, in
    training mode (every call normalises with its own batch's statistics: the same rows) and in eval mode."""
    import torch
    from wholegraph_amd import nn
    n, F, H, N = 1500, 100, 64, 47
    g = torch.Generator(device="cuda").manual_seed(7)
    E = 12000
    ei = torch.stack([torch.randint(0, n, (E,), generator=g, device="cuda"), torch.randint(0, n - 50, (E,), generator=g, device="cuda")])
    ei[1, :300] = ei[0, :300]                      # self loops
    ei = torch.cat([ei, ei[:, 1000:1500]], 1)      # duplicate edges
    conv = _bn_conv(F, H, N, seed=4, eps=-0.1)
    x = torch.randn((n, F), device="cuda")
    order = torch.sort(ei[1], stable=True).indices
    rp = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    rp[1:] = torch.cumsum(torch.bincount(ei[1], minlength=n), 0)
    col = ei[0][order].to(torch.int32).contiguous()
    lg = nn.LayerGraph([nn.HopGraph(rp, col, torch.arange(n, device="cuda"))])
    for mode in ("train", "eval"):
        conv.train(mode == "train")
        with torch.no_grad():
            got = conv(x, ei, act="relu")
            got2 = conv(x, [rp, col], act="relu")
            got3 = conv(x, lg, act="relu")
        assert got.shape == (n, N)
        assert torch.equal(got, got2) and torch.equal(got, got3), mode
    agg, agg_abs = gin_aggregate(x, ei, -0.1), gin_aggregate(x, ei, -0.1, abs_terms=True)
    bn = _parts(conv)[1]
    ref = _Ref(conv, agg, agg_abs, relu=True, stats=(bn.running_mean, bn.running_var))
    _close(got, ref.out, ref.out_abs, "eval, edge_index")
    # gradients through the edge_index path against float64 autograd (training mode)
    conv.train()
    xg = x.clone().requires_grad_(True)
    conv(xg, ei).sum().backward()
    lin1, _, lin2 = _parts(conv)
    xr = x.double().requires_grad_(True)
    a = torch.zeros((n, F), dtype=torch.float64, device="cuda").index_add_(0, ei[1], xr[ei[0]]) + 0.9 * xr
    z = a @ lin1.weight.detach().double().t() + lin1.bias.detach().double()
    y = (z - z.mean(0)) * (z.var(0, unbiased=False) + bn.eps).rsqrt() * bn.weight.detach().double() + bn.bias.detach().double()
    (torch.relu(y) @ lin2.weight.detach().double().t() + lin2.bias.detach().double()).sum().backward()
    assert float((xg.grad.double() - xr.grad).abs().max()) <= 1e-5 * max(1.0, float(xr.grad.abs().max()))


def test_bipartite_pair(hiplib):
    """(x_src, x_dst) with more destinations than sources, and (x_src, None): no root term — training forward against float64,
    and the gradients of both inputs and of eps against float64 autograd."""
    import torch
    F, H, N = 64, 32, 8
    n_src, n_dst, E = 500, 900, 6000
    g = torch.Generator(device="cuda").manual_seed(F)
    ei = torch.stack([torch.randint(0, n_src, (E,), generator=g, device="cuda"), torch.randint(0, n_dst, (E,), generator=g, device="cuda")])
    ei[1, 0] = n_dst - 1
    conv = _bn_conv(F, H, N, seed=5, eps=0.4, train_eps=True)
    lin1, bn, lin2 = _parts(conv)
    xs, xt = torch.randn((n_src, F), device="cuda"), torch.randn((n_dst, F), device="cuda")
    with torch.no_grad():
        got = conv((xs, xt), ei)
        got_none = conv((xs, None), ei, act="relu")
    assert got.shape == (n_dst, N) and got_none.shape == (n_dst, N) and int(bn.num_batches_tracked) == 2
    ref = _Ref(conv, gin_aggregate(xs, ei, 0.4, x_dst=xt), gin_aggregate(xs, ei, 0.4, x_dst=xt, abs_terms=True))
    _close(got, ref.out, ref.out_abs, "pair")
    ref = _Ref(conv, gin_aggregate(xs, ei, 0.4, root=False), gin_aggregate(xs, ei, 0.4, root=False, abs_terms=True), relu=True)
    _close(got_none, ref.out, ref.out_abs, "no root")
    a, b = xs.clone().requires_grad_(True), xt.clone().requires_grad_(True)
    R = torch.randn((n_dst, N), device="cuda")
    (conv((a, b), ei) * R).sum().backward()
    a64, b64 = xs.double().requires_grad_(True), xt.double().requires_grad_(True)
    e64 = torch.tensor(0.4, dtype=torch.float64, device="cuda", requires_grad=True)
    agg = torch.zeros((n_dst, F), dtype=torch.float64, device="cuda").index_add_(0, ei[1], a64[ei[0]]) + (1 + e64) * b64
    z = agg @ lin1.weight.detach().double().t() + lin1.bias.detach().double()
    y = (z - z.mean(0)) * (z.var(0, unbiased=False) + bn.eps).rsqrt() * bn.weight.detach().double() + bn.bias.detach().double()
    ((torch.relu(y) @ lin2.weight.detach().double().t() + lin2.bias.detach().double()) * R.double()).sum().backward()
    for got_g, want, what in ((a.grad, a64.grad, "dx_src"), (b.grad, b64.grad, "dx_dst"), (conv.eps.grad, e64.grad.reshape(1), "d eps")):
        assert float((got_g.double() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max())), what


def test_misaligned_batch_norm_vectors_fall_back(hiplib, launches):
    """gamma a view into a flat parameter buffer at a 4-B offset: the batch-norm kernels read [H] vectors as float4, so the layer
    takes the aggregate kernel and the MLP's own forward — forward and backward run, none of the route's launches is made."""
    import torch
    F, H, N, n_src = 64, 32, 8, 600
    rp, col, self_rows = _hop(300, n_src, 10, seed=8)
    lg = _layer_graph((rp, col, self_rows))
    conv = _bn_conv(F, H, N, seed=9, eps=0.2)
    lin1, bn, lin2 = _parts(conv)
    flat = torch.empty(H + 4, device="cuda")
    flat[1:H + 1] = bn.weight.detach()
    bn.weight = torch.nn.Parameter(flat[1:H + 1])
    assert bn.weight.data_ptr() % 16 == 4 and conv.route == "mlp_bn"
    x = torch.randn((n_src, F), device="cuda")
    out = conv(x, lg)
    out.sum().backward()
    assert launches == {"gin_layer_forward": 0, "gin_layer_stats": 0, "bn_finalize": 0, "bn_act_linear": 0}
    assert bn.weight.grad is not None and lin1.weight.grad is not None and int(bn.num_batches_tracked) == 1
    ref = _hop_ref(conv, x, rp, col, self_rows, 0.2)
    _close(out.detach(), ref.out, ref.out_abs, "fallback forward")
    conv.eval()
    with torch.no_grad():
        assert conv(x, lg).shape == (300, N)
