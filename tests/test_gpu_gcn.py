"""GPU parity of wholegraph_amd.nn.GCNConv (csrc/wg_gcn.hip): the one-kernel layer, its weight / bias / input gradients, the
edge_index path and the call-group route, against the float64 restatement of torch_geometric.nn.GCNConv (tests/gcn_ref.py) —
|err| <= 1e-5 x the magnitude sum of the terms, and 1e-5 relative on the elements that are not cancellations."""
import pytest

from gcn_ref import gcn_forward, gcn_norm, propagate

pytestmark = pytest.mark.gpu


def _close(got, ref, scale, what):
    import torch
    got, ref, scale = got.double().cpu(), ref.double().cpu(), scale.double().cpu()
    err = (got - ref).abs()
    assert bool((err <= 1e-5 * scale + 1e-7).all()), (what, float((err - 1e-5 * scale).max()))
    big = (ref.abs() >= 0.1 * scale) & (scale > 0)
    if int(big.sum()) > 0:
        assert float((err[big] / ref.abs()[big]).max()) <= 1e-5, what
    assert bool(torch.isfinite(got).all()), what


def _hop(n_dst, n_src, max_deg, seed, loops=True):
    """A sampled-hop-like CSR: degrees 0 .. max_deg (rows of degree 0 included), hub sources, sampled self loops (col equal to
    the destination's own input row) on some rows and duplicate edges."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    deg = torch.randint(0, max_deg + 1, (n_dst,), generator=g, device="cuda")
    deg[:3] = torch.tensor([0, 1, max_deg], device="cuda")
    rp = torch.zeros(n_dst + 1, dtype=torch.int32, device="cuda")
    rp[1:] = torch.cumsum(deg, 0)
    E = int(rp[-1])
    col = torch.randint(0, n_src, (E,), generator=g, device="cuda", dtype=torch.int32)
    u = torch.rand(E, generator=g, device="cuda")
    col[u < 0.1] = 5
    self_rows = torch.randperm(n_src, generator=g, device="cuda")[:n_dst].contiguous()
    if loops and E > 0:
        dst_of = torch.repeat_interleave(torch.arange(n_dst, device="cuda"), deg)
        pick = torch.rand(E, generator=g, device="cuda") < 0.08
        col[pick] = self_rows[dst_of[pick]].to(torch.int32)
    return rp, col, self_rows


def _layer_graph(rp, col, self_rows, n_src):
    from wholegraph_amd import nn
    hop = nn.HopGraph(rp, col, self_rows)
    lg = nn.LayerGraph([hop])
    lg.degree_source = lambda: ([hop], [-1], n_src)      # the hop's destinations are all the rows that have in-edges
    return lg


def _edge_index(rp, col, self_rows):
    import torch
    deg = (rp[1:] - rp[:-1]).long()
    dst = self_rows[torch.repeat_interleave(torch.arange(rp.shape[0] - 1, device="cuda"), deg)]
    return torch.stack([col.long(), dst])


def _conv(F, N, seed, **kw):
    import torch
    from wholegraph_amd import nn
    torch.manual_seed(seed)
    conv = nn.GCNConv(F, N, **kw).cuda()
    with torch.no_grad():
        if conv.bias is not None:
            conv.bias.uniform_(-0.5, 0.5)
    return conv


SHAPES = [(100, 256), (128, 256), (256, 256), (256, 47), (100, 47), (64, 16), (4, 1)]


@pytest.mark.parametrize("F,N", SHAPES + [(300, 64)])
@pytest.mark.parametrize("ids", [None, "int32", "int64"])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("improved", [False, True])
def test_layer_forward_vs_fp64(hiplib, F, N, ids, relu, improved):
    """(a) the layer over a hop with rows of degree 0, sampled loops and duplicates, x a tensor or read through a node list
    (LazyRows, int32 / int64 ids); F = 300 lies outside the kernel's domain (normalised-aggregate kernel + library GEMM)."""
    import torch
    from wholegraph_amd import nn
    n_src, n_dst = 3000, 1700
    rp, col, self_rows = _hop(n_dst, n_src, 24, seed=F + N)
    table = torch.randn((5000, F), device="cuda")
    if ids is None:
        x, xd = table[:n_src].contiguous(), table[:n_src]
    else:
        idv = torch.randperm(5000, device="cuda")[:n_src].to(getattr(torch, ids))
        x, xd = nn.LazyRows(table, idv), table[idv.long()]
    conv = _conv(F, N, seed=1, improved=improved)
    with torch.no_grad():
        got = conv(x, _layer_graph(rp, col, self_rows, n_src), act="relu" if relu else None)
    ei = _edge_index(rp, col, self_rows)
    kw = dict(improved=improved)
    ref = gcn_forward(xd.double(), ei, conv.lin.weight.detach(), conv.bias.detach(), relu=relu, **kw)[self_rows]
    scale = gcn_forward(xd.double(), ei, conv.lin.weight.detach(), conv.bias.detach(), abs_terms=True, **kw)[self_rows]
    assert got.shape == (n_dst, N)
    _close(got, ref, scale, "forward")


@pytest.mark.parametrize("F,N", SHAPES + [(300, 64)])
@pytest.mark.parametrize("relu", [False, True])
def test_layer_backward_vs_fp64_and_deterministic(hiplib, F, N, relu):
    """(b) dW, db and dX against float64, and two backward passes bit for bit the same."""
    import torch
    n_src, n_dst = 2600, 1500
    rp, col, self_rows = _hop(n_dst, n_src, 20, seed=3 * F + N)
    conv = _conv(F, N, seed=2)
    x0 = torch.randn((n_src, F), device="cuda")
    R = torch.randn((n_dst, N), device="cuda")
    lg = _layer_graph(rp, col, self_rows, n_src)
    grads = []
    for _ in range(2):
        conv.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        out = conv(x, lg, act="relu" if relu else None)
        (out * R).sum().backward()
        grads.append((conv.lin.weight.grad.clone(), conv.bias.grad.clone(), x.grad.clone(), out.detach().clone()))
    for a, b in zip(grads[0], grads[1]):
        assert torch.equal(a, b), "backward is not run-to-run deterministic"
    gw, gb, gx, out = grads[0]
    src, dst, coef = gcn_norm(_edge_index(rp, col, self_rows), n_src)
    xd = x0.double()
    W = conv.lin.weight.detach().double()
    agg = propagate(src, dst, coef, xd)[self_rows]                     # [n_dst, F]
    agg_abs = propagate(src, dst, coef.abs(), xd.abs())[self_rows]
    dz = R.double() * ((out > 0).double() if relu else 1.0)           # the ReLU mask of the layer's own output
    _close(gw, dz.t() @ agg, dz.abs().t() @ agg_abs, "dW")
    _close(gb, dz.sum(0), dz.abs().sum(0), "db")
    full = torch.zeros((n_src, F), dtype=torch.float64, device="cuda")
    full_abs = torch.zeros_like(full)
    full[self_rows], full_abs[self_rows] = dz @ W, dz.abs() @ W.abs()
    # dX = A_hat^T (dZ W): the transposed propagation
    _close(gx, propagate(dst, src, coef, full), propagate(dst, src, coef.abs(), full_abs), "dX")


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("F,N,kw", [(100, 64, {}), (64, 47, {"improved": True}), (32, 16, {"add_self_loops": False}),
                                    (32, 16, {"normalize": False}), (300, 20, {})])
def test_edge_index_path_vs_fp64(hiplib, weighted, F, N, kw):
    """(c) the ``for batch in loader`` call shape: COO edge_index with duplicates and self loops, with and without edge_weight,
    against PyG's formulation; the [row_ptr, col] CSR pair gives the same rows."""
    import torch
    n = 2500
    g = torch.Generator(device="cuda").manual_seed(F + N)
    E = 30000
    ei = torch.stack([torch.randint(0, n, (E,), generator=g, device="cuda"), torch.randint(0, n - 50, (E,), generator=g, device="cuda")])
    ei[1, :300] = ei[0, :300]                      # self loops
    ei = torch.cat([ei, ei[:, 1000:1500]], 1)      # duplicate edges
    w = torch.rand(ei.shape[1], generator=g, device="cuda") + 0.25 if weighted else None
    if weighted:                                   # (one loop edge per looped node: PyG keeps an arbitrary one of several)
        first = torch.zeros(n, dtype=torch.bool, device="cuda")
        keep = torch.ones(ei.shape[1], dtype=torch.bool, device="cuda")
        for e in torch.nonzero(ei[0] == ei[1]).flatten().tolist():
            v = int(ei[0, e])
            keep[e] = not bool(first[v])
            first[v] = True
        ei, w = ei[:, keep], w[keep]
    conv = _conv(F, N, seed=4, **kw)
    x = torch.randn((n, F), device="cuda")
    with torch.no_grad():
        got = conv(x, ei, edge_weight=w)
    ref = gcn_forward(x.double(), ei, conv.lin.weight.detach(), conv.bias.detach(), edge_weight=w, **kw)
    scale = gcn_forward(x.double(), ei, conv.lin.weight.detach(), conv.bias.detach(), edge_weight=w, abs_terms=True, **kw)
    assert got.shape == (n, N)
    _close(got, ref, scale, "edge_index")
    # the CSR pair (destination-major, edge order kept): same rows
    order = torch.sort(ei[1], stable=True).indices
    rp = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    rp[1:] = torch.cumsum(torch.bincount(ei[1], minlength=n), 0)
    with torch.no_grad():
        got2 = conv(x, [rp, ei[0][order].to(torch.int32).contiguous()], edge_weight=None if w is None else w[order])
    _close(got2, ref, scale, "csr pair")
    # gradients through the edge_index path
    xg = x.clone().requires_grad_(True)
    conv(xg, ei, edge_weight=w).sum().backward()
    xr = x.double().requires_grad_(True)
    gcn_forward(xr, ei, conv.lin.weight.detach(), conv.bias.detach(), edge_weight=w, **kw).sum().backward()
    assert float((xg.grad.double() - xr.grad).abs().max()) <= 1e-5 * max(1.0, float(xr.grad.abs().max()))


def test_layer_graph_without_degrees_and_capture_refused(hiplib):
    import torch
    from wholegraph_amd import nn
    rp, col, self_rows = _hop(100, 300, 5, seed=1)
    conv = _conv(16, 8, seed=0)
    with pytest.raises(ValueError, match="degree"):
        conv(torch.randn(300, 16, device="cuda"), nn.LayerGraph([nn.HopGraph(rp, col, self_rows)]))
    lg = _layer_graph(rp, col, self_rows, 300)
    with pytest.raises(ValueError, match="edge_weight"):
        conv(torch.randn(300, 16, device="cuda"), lg, edge_weight=torch.ones(col.shape[0], device="cuda"))
    table = torch.randn(500, 16, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError):
        conv(nn.LazyRows(table, torch.arange(300, device="cuda")), lg)
    # under HIP-graph capture (loader.PerBatchStep) the layer refuses, as GATConv does
    import wholegraph_amd.nn as wnn
    orig = wnn._capturing
    wnn._capturing = lambda: True
    try:
        with pytest.raises(RuntimeError, match="capture"):
            conv(torch.randn(300, 16, device="cuda"), lg)
    finally:
        wnn._capturing = orig


def _stores(V, F, seed):
    """A power-law graph with self loops on some vertices and duplicated edges, features on the device."""
    import numpy as np
    import torch
    from cugraph_pyg_amd.data import FeatureStore, GraphStore
    from graphgen import powerlaw_csr
    row_ptr, col = powerlaw_csr(V, 10, seed=seed, max_deg=300)
    dst = np.repeat(np.arange(V), np.diff(row_ptr))
    rng = np.random.default_rng(seed)
    loops = rng.choice(V, V // 5, replace=False)
    dup = rng.choice(col.shape[0], col.shape[0] // 10, replace=False)
    src_all = np.concatenate([col.astype(np.int64), loops, loops[: V // 20], col[dup].astype(np.int64)])
    dst_all = np.concatenate([dst, loops, loops[: V // 20], dst[dup]])
    gs, fs = GraphStore(), FeatureStore()
    gs[("n", "e", "n"), "coo", False, (V, V)] = torch.stack([torch.from_numpy(src_all), torch.from_numpy(dst_all)]).cuda()
    fs["n", "x", None] = torch.from_numpy(rng.standard_normal((V, F)).astype(np.float32)).cuda()
    return gs, fs


@pytest.mark.parametrize("fanout", [[10, 5], [15, 10, 5]])
def test_call_group_gcn_equals_untrimmed_fp64(hiplib, fanout):
    """(d) GCN over a call group's trimmed layer graphs with lazy x equals, at every seed, the untrimmed float64 GCN over its
    own mini-batch (``to_data_list()``: batch.x / batch.edge_index, which hold the sampled self loops and duplicates); the
    gradients of a 2-layer model equal float64 autograd."""
    import torch
    from cugraph_pyg_amd.loader import NeighborLoader
    from wholegraph_amd.nn import LazyRows
    V, F0 = 6000, 64
    gs, fs = _stores(V, F0, seed=17)
    H = len(fanout)
    dims = [F0] + [48] * (H - 1) + [10]
    convs = [_conv(dims[i], dims[i + 1], seed=10 + i) for i in range(H)]
    B, G = 48, 3
    seeds = torch.randperm(V, generator=torch.Generator().manual_seed(2))[:G * B].cuda()
    loader = NeighborLoader((fs, gs), fanout, input_nodes=seeds, batch_size=B, shuffle=False, random_state=7, local_seeds_per_call=G * B)
    grp = next(iter(loader.call_groups()))
    assert isinstance(grp.x, LazyRows)

    def run():
        h = grp.x
        for j, c in enumerate(convs):
            h = c(h, grp.layer_graph(j), act="relu" if j + 1 < H else None)
        return h

    with torch.no_grad():
        got = run()
    datas = grp.to_data_list()

    def ref_forward(params, d, abs_terms=False):
        h = d.x.double().cuda()
        for j, (w, b) in enumerate(params):
            h = gcn_forward(h, d.edge_index, w, b, relu=j + 1 < H, abs_terms=abs_terms)
        return h[:d.batch_size]

    params = [(c.lin.weight.detach(), c.bias.detach()) for c in convs]
    ref = torch.cat([ref_forward(params, d) for d in datas])
    scale = torch.cat([ref_forward(params, d, abs_terms=True) for d in datas])
    assert got.shape == ref.shape
    assert any(bool((d.edge_index[0] == d.edge_index[1]).any()) for d in datas), "no sampled self loop: the case is not covered"
    _close(got, ref, scale, "logits")
    if H != 2:
        return
    R = torch.randn(got.shape, device="cuda")
    (run() * R).sum().backward()
    dbl = [(c.lin.weight.detach().double().requires_grad_(True), c.bias.detach().double().requires_grad_(True)) for c in convs]
    (torch.cat([ref_forward(dbl, d) for d in datas]) * R.double()).sum().backward()
    for c, (w, b) in zip(convs, dbl):
        for got_g, want in ((c.lin.weight.grad, w.grad), (c.bias.grad, b.grad)):
            assert float((got_g.double() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
