"""GPU parity of wholegraph_amd.nn.TransformerConv (csrc/wg_transformer.hip): the one-kernel layer, its parameter / input /
edge-attribute gradients, the edge_index and CSR-pair paths, the call-group route and the link-loader loop, against the
float64 restatement of torch_geometric.nn.TransformerConv (tests/transformer_ref.py) — |err| <= 1e-5 x the magnitude sum
of the terms on the output."""
import pytest

from transformer_ref import params_of, transformer_forward

pytestmark = pytest.mark.gpu


def _close(got, ref, scale, what):
    import torch
    got, ref, scale = got.double().cpu(), ref.double().cpu(), scale.double().cpu()
    assert got.shape == ref.shape, what
    err = (got - ref).abs()
    assert bool((err <= 1e-5 * scale + 1e-7).all()), (what, float((err - 1e-5 * scale).max()))
    assert bool(torch.isfinite(got).all()), what


def _close_grad(got, ref, what, rel=1e-4):
    """A gradient against float64 autograd: max |err| <= rel x max |ref| (the softmax backward cancels term by term)."""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, what
    bar = rel * max(float(ref.abs().max()), 1e-6)
    assert float((got - ref).abs().max()) <= bar, (what, float((got - ref).abs().max()), bar)


def _hop(n_dst, n_src, max_deg, seed, hub=0):
    """A sampled-hop-like CSR: degrees 0 .. max_deg (rows 0 and 3 without edges), hub sources, sampled self loops, duplicate
    edges and, with ``hub``, row 1 of ``hub`` edges."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    deg = torch.randint(0, max_deg + 1, (n_dst,), generator=g, device="cuda")
    deg[0] = 0
    deg[3] = 0
    deg[2] = max_deg
    if hub:
        deg[1] = hub
    rp = torch.zeros(n_dst + 1, dtype=torch.int32, device="cuda")
    rp[1:] = torch.cumsum(deg, 0)
    E = int(rp[-1])
    col = torch.randint(0, n_src, (E,), generator=g, device="cuda", dtype=torch.int32)
    col[torch.rand(E, generator=g, device="cuda") < 0.1] = 5
    # (injective when n_src >= n_dst; a bipartite hop with more destinations than sources ignores self_rows)
    self_rows = (torch.randperm(max(n_src, n_dst), generator=g, device="cuda")[:n_dst] % n_src).contiguous()
    dst_of = torch.repeat_interleave(torch.arange(n_dst, device="cuda"), deg)
    pick = torch.rand(E, generator=g, device="cuda") < 0.08
    col[pick] = self_rows[dst_of[pick]].to(torch.int32)
    return rp, col, self_rows


def _edge_index(rp, self_rows, col):
    import torch
    deg = (rp[1:] - rp[:-1]).long()
    dst = self_rows[torch.repeat_interleave(torch.arange(rp.shape[0] - 1, device="cuda"), deg)]
    return torch.stack([col.long(), dst])


def _count_launches(monkeypatch):
    """A list that gets one entry per ``nn.transformer_layer_forward`` call (one kernel launch per hop)."""
    from wholegraph_amd import nn
    launches = []
    orig = nn.transformer_layer_forward
    monkeypatch.setattr(nn, "transformer_layer_forward", lambda *a, **k: launches.append(1) or orig(*a, **k))
    return launches


def _conv(fin, C, H, concat, D, seed, **kw):
    import torch
    from wholegraph_amd import nn
    torch.manual_seed(seed)
    conv = nn.TransformerConv(fin, C, heads=H, concat=concat, edge_dim=D, **kw).cuda()
    with torch.no_grad():                                  # logits of order 1-10: a softmax that is neither flat nor one-hot
        for lin in (conv.lin_query, conv.lin_key):
            lin.weight.mul_(3.0)
        conv.lin_value.bias.uniform_(-0.5, 0.5)
    return conv


# (heads, concat, edge_dim, (F_src, C), bipartite F_dst or None, lazy ids, relu)
FWD = [(1, False, 1, (64, 64), None, None, False),          # the reference layer
       (1, True, 1, (100, 256), None, "int32", True),        # bench.py's products width
       (4, True, None, (64, 64), None, None, False),          # H = 4 concat, K = 4 ceil4(65) + 64 = 336
       (3, False, 4, (32, 16), None, "int64", True),
       (2, True, 4, (48, 24), 20, None, False),              # bipartite, F_dst != F_src
       (8, True, None, (16, 8), None, None, True),
       (2, False, None, (128, 32), 64, None, False),
       (5, True, 1, (16, 16), None, "int32", False)]


@pytest.mark.parametrize("case", range(len(FWD)))
def test_layer_forward_vs_fp64(hiplib, case, monkeypatch):
    """(a) the layer over a hop with rows of degree 0, loops, duplicates and one row of 3000 edges (the online softmax over
    many groups): heads, concat, edge_dim in {None, 1, 4}, bipartite input (COO, x = (x_src, x_dst)), a lazy x (LazyRows
    with int32 / int64 ids) and relu rotate through the cases; alpha (return_attention_weights) against the restatement's.
    Every case runs the kernel — case 6 after copying a float64 x_src and a strided x_dst to float32 rows."""
    import torch
    from wholegraph_amd import nn
    H, concat, D, (F, C), Fd, ids, relu = FWD[case]
    n_src, n_dst = 1600, 700
    rp, col, self_rows = _hop(n_dst, n_src, 24, seed=case, hub=3000)
    E = col.shape[0]
    conv = _conv(F if Fd is None else (F, Fd), C, H, concat, D, seed=case)
    N = H * C if concat else C
    assert nn.transformer_layer_supported(F, F if Fd is None else Fd, D or 0, H, N)
    ea = torch.randn((E, D), device="cuda") if D else None
    act = "relu" if relu else None
    p = params_of(conv)
    launches = _count_launches(monkeypatch)
    if Fd is not None:
        xs = torch.randn((n_src, F), device="cuda")
        xd = torch.randn((n_dst, Fd), device="cuda")
        if case == 6:
            xs = xs.double()
            xd = torch.stack([xd, torch.randn_like(xd)], 2).view(n_dst, 2 * Fd)[:, ::2]    # stride (2 Fd, 2)
        ei = _edge_index(rp, torch.arange(n_dst, device="cuda"), col)
        with torch.no_grad():
            got, (ei2, alpha) = conv((xs, xd), ei, ea, act=act, return_attention_weights=True)
        assert ei2 is ei
        ref, ra = transformer_forward(xs, xd, ei, p, H, concat, ea, relu=relu, return_alpha=True)
        scale = transformer_forward(xs, xd, ei, p, H, concat, ea, abs_terms=True)
    else:
        table = torch.randn((3000, F), device="cuda")
        if ids is None:
            x, xd64 = table[:n_src].contiguous(), table[:n_src]
        else:
            idv = torch.randperm(3000, device="cuda")[:n_src].to(getattr(torch, ids))
            x, xd64 = nn.LazyRows(table, idv), table[idv.long()]
        ei = _edge_index(rp, self_rows, col)
        with torch.no_grad():
            got, alpha = conv(x, nn.LayerGraph([nn.HopGraph(rp, col, self_rows)]), ea, act=act, return_attention_weights=True)
        ref, ra = transformer_forward(xd64, None, ei, p, H, concat, ea, relu=relu, return_alpha=True)
        scale = transformer_forward(xd64, None, ei, p, H, concat, ea, abs_terms=True)
        ref, scale = ref[self_rows], scale[self_rows]
    assert got.shape == (n_dst, N)
    assert len(launches) == 1, "the one-kernel route"
    _close(got, ref, scale, "forward")
    assert float((alpha.double() - ra).abs().max()) <= 1e-5, "alpha"


# (heads, concat, edge_dim, (F_src, C), bipartite F_dst or None, relu, lazy ids, (n_src, n_dst))
BWD = [(1, False, 1, (64, 64), None, True), (4, True, None, (64, 64), None, False), (3, False, 4, (32, 16), None, True),
       (2, True, 4, (48, 24), 20, False), (1, True, 1, (100, 256), None, True), (2, True, 1, (32, 16), None, False, "int32"),
       (2, True, 4, (48, 24), 20, True, None, (300, 700))]        # bipartite with more destinations than sources


@pytest.mark.parametrize("case", range(len(BWD)))
def test_layer_backward_vs_fp64_and_deterministic(hiplib, case, monkeypatch):
    """(b) every parameter gradient and the gradients of x (x_src and x_dst when bipartite) and edge_attr against float64
    autograd of the restatement; lin_key.bias's gradient is zero (it cancels in the softmax).  Two backward passes give the
    same bits, on the kernel route.  Case 5 reads x through LazyRows (no dx); case 6 is bipartite with 300 source rows
    and 700 destinations."""
    import torch
    from wholegraph_amd import nn
    H, concat, D, (F, C), Fd, relu = BWD[case][:6]
    ids = BWD[case][6] if len(BWD[case]) > 6 else None
    n_src, n_dst = BWD[case][7] if len(BWD[case]) > 7 else (1500, 600)
    launches = _count_launches(monkeypatch)
    rp, col, self_rows = _hop(n_dst, n_src, 20, seed=10 + case, hub=1500)
    E = col.shape[0]
    conv = _conv(F if Fd is None else (F, Fd), C, H, concat, D, seed=20 + case)
    N = H * C if concat else C
    x0 = torch.randn((n_src, F), device="cuda")
    xd0 = torch.randn((n_dst, Fd), device="cuda") if Fd else None
    ea0 = torch.randn((E, D), device="cuda") if D else None
    G = torch.randn((n_dst, N), device="cuda")
    lg = nn.LayerGraph([nn.HopGraph(rp, col, self_rows)])
    ei = _edge_index(rp, self_rows if Fd is None else torch.arange(n_dst, device="cuda"), col)
    if ids is not None:
        idv = torch.randperm(n_src, device="cuda").to(getattr(torch, ids))
        table = torch.empty_like(x0)
        table[idv.long()] = x0
    runs = []
    act = "relu" if relu else None
    for _ in range(2):
        conv.zero_grad(set_to_none=True)
        ea = None if ea0 is None else ea0.clone().requires_grad_(True)
        if Fd is not None:
            xs, xd = x0.clone().requires_grad_(True), xd0.clone().requires_grad_(True)
            out = conv((xs, xd), ei, ea, act=act)
            xg = [xs, xd]
        elif ids is not None:
            out = conv(nn.LazyRows(table, idv), lg, ea, act=act)
            xg = []
        else:
            xs = x0.clone().requires_grad_(True)
            out = conv(xs, lg, ea, act=act)
            xg = [xs]
        (out * G).sum().backward()
        grads = {k: p.grad.clone() for k, p in conv.named_parameters()}
        for k, t in enumerate(xg):
            grads["x%d" % k] = t.grad.clone()
        if ea is not None:
            grads["edge_attr"] = ea.grad.clone()
        runs.append((out.detach().clone(), grads))
    assert len(launches) == 2, "the one-kernel route"
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), "backward is not run-to-run deterministic: " + k
    assert torch.equal(runs[0][0], runs[1][0])
    p64 = {k: None if v is None else v.double().requires_grad_(True) for k, v in params_of(conv).items()}
    x64 = x0.double().requires_grad_(True)
    xd64 = None if xd0 is None else xd0.double().requires_grad_(True)
    ea64 = None if ea0 is None else ea0.double().requires_grad_(True)
    ref = transformer_forward(x64, xd64, ei, p64, H, concat, ea64, relu=relu)
    if Fd is None:
        ref = ref[self_rows]
    (ref * G.double()).sum().backward()
    names = {"lin_query.weight": "Wq", "lin_query.bias": "bq", "lin_key.weight": "Wk", "lin_value.weight": "Wv",
             "lin_value.bias": "bv", "lin_edge.weight": "We", "lin_skip.weight": "Ws", "lin_skip.bias": "bs"}
    got = runs[0][1]
    for k, r in names.items():
        if k in got:
            _close_grad(got[k], p64[r].grad, "d" + k)
    assert float(got["lin_key.bias"].abs().max()) <= 1e-4 * float(got["lin_key.weight"].abs().max()), "dlin_key.bias"
    if ids is None:
        _close_grad(got["x0"], x64.grad, "dx")
    if Fd is not None:
        _close_grad(got["x1"], xd64.grad, "dx_dst")
    if D:
        _close_grad(got["edge_attr"], ea64.grad, "dedge_attr")


@pytest.mark.parametrize("H,concat,D", [(1, False, 1), (2, True, 3)])
def test_edge_index_and_csr_pair_paths(hiplib, H, concat, D):
    """(c) the ``for batch in loader`` call shape: COO edge_index with duplicates, loops and a hub of 3000 in-edges; the
    [row_ptr, col] CSR pair with edge_attr in CSR order gives the same rows; alpha comes back in edge_index order."""
    import torch
    n, F, C = 2000, 32, 16
    g = torch.Generator(device="cuda").manual_seed(H + D)
    E = 20000
    ei = torch.stack([torch.randint(0, n, (E,), generator=g, device="cuda"), torch.randint(0, n - 50, (E,), generator=g, device="cuda")])
    ei[1, :3000] = 7
    ei[1, 3000:3300] = ei[0, 3000:3300]
    ei = torch.cat([ei, ei[:, 5000:5500]], 1)
    ea = torch.randn((ei.shape[1], D), generator=g, device="cuda")
    conv = _conv(F, C, H, concat, D, seed=4)
    x = torch.randn((n, F), device="cuda")
    p = params_of(conv)
    with torch.no_grad():
        got, (_, alpha) = conv(x, ei, ea, return_attention_weights=True)
    ref, ra = transformer_forward(x, None, ei, p, H, concat, ea, return_alpha=True)
    scale = transformer_forward(x, None, ei, p, H, concat, ea, abs_terms=True)
    _close(got, ref, scale, "edge_index")
    assert float((alpha.double() - ra).abs().max()) <= 1e-5
    order = torch.sort(ei[1], stable=True).indices
    rp = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    rp[1:] = torch.cumsum(torch.bincount(ei[1], minlength=n), 0)
    with torch.no_grad():
        got2 = conv(x, [rp, ei[0][order].to(torch.int32).contiguous()], ea[order])
    _close(got2, ref, scale, "csr pair")
    # a destination-sorted edge_index with the loader's marker: taken in its own order, the same rows and alpha as the unsorted list
    ei_s = ei[:, order].contiguous()
    ei_s._wgamd_dst_sorted = ei_s._version
    with torch.no_grad():
        got3, (_, alpha3) = conv(x, ei_s, ea[order], return_attention_weights=True)
    assert torch.equal(got3, got) and torch.equal(alpha3, alpha[order])


def test_bad_edge_attr_and_fallback(hiplib, monkeypatch):
    """(f) a bad edge_attr (missing, wrong length, width, dtype or device) raises ValueError before any launch; (g) a shape
    outside the kernel's domain (F = 30) runs library ops and still matches float64, forward and gradients."""
    import torch
    from wholegraph_amd import nn
    rp, col, self_rows = _hop(100, 300, 5, seed=1)
    E = col.shape[0]
    conv = _conv(16, 8, 2, True, 2, seed=0)
    x = torch.randn(300, 16, device="cuda")
    lg = nn.LayerGraph([nn.HopGraph(rp, col, self_rows)])
    ea = torch.randn(E, 2, device="cuda")
    launches = []
    orig = nn.transformer_layer_forward
    monkeypatch.setattr(nn, "transformer_layer_forward", lambda *a, **k: launches.append(1) or orig(*a, **k))
    for bad, what in [(None, "needs edge_attr"), (ea[:-1], "rows"), (torch.randn(E, 3, device="cuda"), "shape"),
                      (ea.to(torch.int32), "floating"), (ea.cpu(), "cpu")]:
        with pytest.raises(ValueError, match=what):
            conv(x, lg, bad)
    ei = _edge_index(rp, self_rows, col)
    with pytest.raises(ValueError, match="rows"):
        conv(x, ei, ea[1:])
    assert not launches
    conv(x, lg, ea)
    assert launches
    # out of the domain: F = 30 (not a multiple of 4) -> library ops
    calls = []
    orig_lib = nn._tconv_library_ops
    monkeypatch.setattr(nn, "_tconv_library_ops", lambda *a, **k: calls.append(1) or orig_lib(*a, **k))
    c30 = _conv(30, 12, 2, False, 1, seed=3)
    assert not nn.transformer_layer_supported(30, 30, 1, 2, 12)
    x30 = torch.randn(300, 30, device="cuda", requires_grad=True)
    ea1 = torch.randn(E, 1, device="cuda")
    out = c30(x30, lg, ea1, act="relu")
    assert calls
    p = params_of(c30)
    _close(out.detach(), transformer_forward(x30.detach(), None, ei, p, 2, False, ea1, relu=True)[self_rows],
           transformer_forward(x30.detach(), None, ei, p, 2, False, ea1, abs_terms=True)[self_rows], "fallback")
    out.sum().backward()
    x64 = x30.detach().double().requires_grad_(True)
    transformer_forward(x64, None, ei, p, 2, False, ea1, relu=True)[self_rows].sum().backward()
    _close_grad(x30.grad, x64.grad, "fallback dx")


def _stores(V, F, D, seed):
    """A power-law graph with self loops and duplicated edges, node features and a [E, D] edge attribute on the device."""
    import numpy as np
    import torch
    from cugraph_pyg_amd.data import FeatureStore, GraphStore
    from graphgen import powerlaw_csr
    row_ptr, col = powerlaw_csr(V, 10, seed=seed, max_deg=300)
    dst = np.repeat(np.arange(V), np.diff(row_ptr))
    rng = np.random.default_rng(seed)
    loops = rng.choice(V, V // 5, replace=False)
    dup = rng.choice(col.shape[0], col.shape[0] // 10, replace=False)
    src_all = np.concatenate([col.astype(np.int64), loops, col[dup].astype(np.int64)])
    dst_all = np.concatenate([dst, loops, dst[dup]])
    gs, fs = GraphStore(), FeatureStore()
    gs[("n", "e", "n"), "coo", False, (V, V)] = torch.stack([torch.from_numpy(src_all), torch.from_numpy(dst_all)]).cuda()
    fs["n", "x", None] = torch.from_numpy(rng.standard_normal((V, F)).astype(np.float32)).cuda()
    attr = torch.from_numpy(rng.standard_normal((src_all.shape[0], D)).astype(np.float32)).cuda()
    fs[("n", "e", "n"), "attr", None] = attr
    return gs, fs, attr


@pytest.mark.parametrize("fanout", [[10, 5], [15, 10, 5]])
def test_call_group_equals_per_batch_fp64(hiplib, fanout):
    """(d) a stack of TransformerConv over a call group's trimmed layer graphs (lazy x, edge_attr = cg.edge_attr("attr") for every
    layer) equals, at every seed, the float64 restatement run on each mini-batch of ``to_data_list()`` with
    ``attr[batch.e_id]``."""
    import torch
    from cugraph_pyg_amd.loader import NeighborLoader
    V, F0 = 6000, 32
    gs, fs, attr = _stores(V, F0, 1, seed=23)
    L_ = len(fanout)
    convs = [_conv(F0 if i == 0 else 32, 32 if i + 1 < L_ else 8, 1 if i % 2 == 0 else 2, i % 2 == 0, 1, seed=30 + i)
             for i in range(L_)]
    B, G = 48, 3
    seeds = torch.randperm(V, generator=torch.Generator().manual_seed(2))[:G * B].cuda()
    loader = NeighborLoader((fs, gs), fanout, input_nodes=seeds, batch_size=B, shuffle=False, random_state=7,
                            local_seeds_per_call=G * B)
    grp = next(iter(loader.call_groups()))
    ea = grp.edge_attr("attr")
    assert torch.equal(ea, attr[grp.e_id])
    with torch.no_grad():
        h = grp.x
        for j, c in enumerate(convs):
            h = c(h, grp.layer_graph(j), ea, act="relu" if j + 1 < L_ else None)
    refs, scales = [], []
    for d in grp.to_data_list():
        r = d.x.double().cuda()
        s = None
        ed = attr[d.e_id.cuda()]
        for j, c in enumerate(convs):
            p = params_of(c)
            if j + 1 == L_:
                s = transformer_forward(r, None, d.edge_index, p, c.heads, c.concat, ed, abs_terms=True)
            r = transformer_forward(r, None, d.edge_index, p, c.heads, c.concat, ed, relu=j + 1 < L_)
        refs.append(r[:d.batch_size])
        scales.append(s[:d.batch_size])
    ref, scale = torch.cat(refs), torch.cat(scales)
    assert h.shape == ref.shape
    # (the scale of the last layer's terms; earlier layers' rounding enters through its input: a looser bar)
    _close(h, ref, 10 * scale, "logits")


def test_link_loader_loop_forward_backward(hiplib):
    """(e) the reference example's loop: ``for batch in LinkNeighborLoader(...)`` with ``conv(x, batch.edge_index,
    attr[batch.e_id])`` over a trainable embedding — forward equal to float64, backward with finite gradients everywhere."""
    import torch
    from cugraph_pyg_amd.loader import LinkNeighborLoader
    V = 3000
    gs, fs, attr = _stores(V, 8, 1, seed=5)
    emb = torch.nn.Parameter(torch.randn(V, 64, device="cuda"))
    convs = [_conv(64, 64, 1, False, 1, seed=40), _conv(64, 64, 1, False, 1, seed=41)]
    src = torch.randint(0, V, (400,), generator=torch.Generator().manual_seed(3)).cuda()
    dst = torch.randint(0, V, (400,), generator=torch.Generator().manual_seed(4)).cuda()
    loader = LinkNeighborLoader((fs, gs), [10, 5], edge_label_index=torch.stack([src, dst]), batch_size=200, random_state=3)
    n = 0
    for batch in loader:
        x = emb[batch.n_id.cuda()]
        ea = attr[batch.e_id.cuda()]
        h = convs[0](x, batch.edge_index, ea, act="relu")
        h = convs[1](h, batch.edge_index, ea)
        with torch.no_grad():
            r = transformer_forward(x, None, batch.edge_index, params_of(convs[0]), 1, False, ea, relu=True)
            r = transformer_forward(r, None, batch.edge_index, params_of(convs[1]), 1, False, ea)
        assert float((h.detach().double() - r).abs().max()) <= 1e-4 * max(1.0, float(r.abs().max()))
        h.square().mean().backward()
        n += 1
    assert n == 2
    assert emb.grad is not None and bool(torch.isfinite(emb.grad).all()) and float(emb.grad.abs().sum()) > 0
    for c in convs:
        for name, p in c.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
