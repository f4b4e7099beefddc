"""GPU parity of wholegraph_amd.nn.RGCNConv (csrc/wg_rgcn.hip): the one-kernel layer, its weight / basis / comp / root / bias /
input gradients, the edge_index and CSR-pair paths, the call-group route and CallGroup.edge_attr, against the float64
restatement of torch_geometric.nn.RGCNConv (tests/rgcn_ref.py) — |err| <= 1e-5 x the magnitude sum of the terms, and 1e-5
relative on the elements that are not cancellations."""
import itertools

import pytest

from rgcn_ref import rgcn_forward

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


def _hop(n_dst, n_src, max_deg, R, seed):
    """A sampled-hop-like CSR: degrees 0 .. max_deg, hub sources, sampled self loops (col = the destination's own input row),
    duplicate edges, rows with a single relation; relation ids uniform in [0, R)."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    deg = torch.randint(0, max_deg + 1, (n_dst,), generator=g, device="cuda")
    deg[:3] = torch.tensor([0, 1, max_deg], device="cuda")
    rp = torch.zeros(n_dst + 1, dtype=torch.int32, device="cuda")
    rp[1:] = torch.cumsum(deg, 0)
    E = int(rp[-1])
    col = torch.randint(0, n_src, (E,), generator=g, device="cuda", dtype=torch.int32)
    col[torch.rand(E, generator=g, device="cuda") < 0.1] = 5
    self_rows = torch.randperm(n_src, generator=g, device="cuda")[:n_dst].contiguous()
    dst_of = torch.repeat_interleave(torch.arange(n_dst, device="cuda"), deg)
    pick = torch.rand(E, generator=g, device="cuda") < 0.08
    col[pick] = self_rows[dst_of[pick]].to(torch.int32)
    et = torch.randint(0, R, (E,), generator=g, device="cuda")
    single = (dst_of % 7) == 3                     # every edge of these rows carries the same relation
    et[single] = (dst_of[single] % R)
    return rp, col, self_rows, et


def _edge_index(rp, self_rows, col):
    import torch
    deg = (rp[1:] - rp[:-1]).long()
    dst = self_rows[torch.repeat_interleave(torch.arange(rp.shape[0] - 1, device="cuda"), deg)]
    return torch.stack([col.long(), dst])


def _conv(F, N, R, bases, seed, **kw):
    import torch
    from wholegraph_amd import nn
    torch.manual_seed(seed)
    conv = nn.RGCNConv(F, N, R, num_bases=bases, **kw).cuda()
    with torch.no_grad():
        if conv.bias is not None:
            conv.bias.uniform_(-0.5, 0.5)
    return conv


def _params(conv):
    d = lambda p: None if p is None else p.detach()   # noqa: E731
    return dict(weight=d(conv.weight), comp=d(conv.comp), root=d(conv.root), bias=d(conv.bias))


GRID = list(itertools.product([None, 4, 30], [1, 3, 535], [(32, 32), (100, 64), (64, 47), (128, 256)]))
VARIANTS = list(itertools.product([None, "int32", "int64"], [False, True], ["mean", "add"]))


@pytest.mark.parametrize("case", range(len(GRID) + 1))
def test_layer_forward_vs_fp64(hiplib, case):
    """(a) the layer over a hop with rows of degree 0, loops, duplicates and single-relation rows, over bases x R x (F, N); the
    node-list kind (x a tensor, or LazyRows with int32 / int64 ids), relu and aggr rotate through the cases.  The last case is
    the out-of-domain shape F = 30 (not a multiple of 4): library ops over the same coefficients."""
    import torch
    from wholegraph_amd import nn
    bases, R, (F, N) = GRID[case] if case < len(GRID) else (None, 535, (30, 20))
    ids, relu, aggr = VARIANTS[case % len(VARIANTS)]
    n_src, n_dst = 1600, 900
    rp, col, self_rows, et = _hop(n_dst, n_src, 24, R, seed=case)
    if case % 2:
        et = et.to(torch.int32)
    table = torch.randn((3000, F), device="cuda")
    if ids is None:
        x, xd = table[:n_src].contiguous(), table[:n_src]
    else:
        idv = torch.randperm(3000, device="cuda")[:n_src].to(getattr(torch, ids))
        x, xd = nn.LazyRows(table, idv), table[idv.long()]
    conv = _conv(F, N, R, bases, seed=case, aggr=aggr)
    assert nn.rgcn_layer_supported(F, N, bases or R, True) == (F % 4 == 0 and ((bases or R) + 1) * F <= 1024)
    with torch.no_grad():
        got = conv(x, nn.LayerGraph([nn.HopGraph(rp, col, self_rows)]), et, act="relu" if relu else None)
    ei = _edge_index(rp, self_rows, col)
    ref = rgcn_forward(xd.double(), ei, et, relu=relu, aggr=aggr, **_params(conv))[self_rows]
    scale = rgcn_forward(xd.double(), ei, et, aggr=aggr, abs_terms=True, **_params(conv))[self_rows]
    assert got.shape == (n_dst, N)
    _close(got, ref, scale, "forward")


BWD = [(32, 32, 535, 30, True, {}), (32, 32, 3, None, False, {}), (64, 47, 8, 4, True, {}), (100, 64, 8, None, False, {}),
       (60, 16, 535, None, True, {}), (100, 256, 8, None, True, {}),
       (32, 32, 535, 30, True, {"ids": "int32"}), (64, 47, 8, None, False, {"ids": "int64", "aggr": "add"}),
       (32, 16, 5, 4, True, {"root_weight": False, "bias": False}), (48, 32, 3, None, False, {"root_weight": False, "aggr": "add"})]


@pytest.mark.parametrize("F,N,R,bases,relu,kw", BWD)
def test_layer_backward_vs_fp64_and_deterministic(hiplib, F, N, R, bases, relu, kw, monkeypatch):
    """(b) dx, dweight, dcomp, droot and dbias against float64 autograd of the restatement, and two backward passes bit for bit
    the same on the kernel route.  The route: the one-kernel layer when the forward shape is in the domain and, if x needs a
    gradient, the transposed shape (F' = N rounded up to 4, N' = F) is too; otherwise the whole layer runs library ops.
    (100, 64, R = 8): both directions in the kernel ((8 + 1) x 64 <= 1024); (100, 256, R = 8): the forward shape fits but the
    input gradient's does not ((8 + 1) x 256 > 1024), so library ops; (60, 16, 535): library ops (F % 4 != 0).  With ``ids`` x
    is LazyRows (no dx; the weight gradient reads the rows through the node list), and root_weight / bias / aggr vary."""
    import torch
    from wholegraph_amd import nn
    n_src, n_dst = 1500, 800
    ids, kw = kw.get("ids"), {k: v for k, v in kw.items() if k != "ids"}
    rp, col, self_rows, et = _hop(n_dst, n_src, 20, R, seed=F + N + R)
    conv = _conv(F, N, R, bases, seed=2, **kw)
    has_root = conv.root is not None
    x0 = torch.randn((n_src, F), device="cuda")
    G = torch.randn((n_dst, N), device="cuda")
    lg = nn.LayerGraph([nn.HopGraph(rp, col, self_rows)])
    if ids is not None:
        table = torch.randn((n_src + 500, F), device="cuda")
        idv = torch.randperm(n_src + 500, device="cuda")[:n_src].to(getattr(torch, ids))
        x0 = table[idv.long()]
    kernel = nn.rgcn_layer_supported(F, N, bases or R, has_root) and (
        ids is not None or nn.rgcn_layer_supported((N + 3) // 4 * 4, F, bases or R, has_root))
    lib_calls = []
    orig = nn._rgcn_library_ops
    monkeypatch.setattr(nn, "_rgcn_library_ops", lambda *a, **k: lib_calls.append(1) or orig(*a, **k))
    names = [k for k in ("weight", "comp", "root", "bias") if getattr(conv, k) is not None]
    runs = []
    for _ in range(2):
        conv.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True) if ids is None else nn.LazyRows(table, idv)
        out = conv(x, lg, et, act="relu" if relu else None)
        (out * G).sum().backward()
        runs.append([getattr(conv, k).grad.clone() for k in names] + [x.grad.clone() if ids is None else None, out.detach().clone()])
    assert bool(lib_calls) == (not kernel), "route"
    if kernel:
        for a, b in zip(runs[0], runs[1]):
            assert a is None or torch.equal(a, b), "backward is not run-to-run deterministic"
    ei = _edge_index(rp, self_rows, col)
    aggr = kw.get("aggr", "mean")
    none = {k: None for k in ("comp", "root", "bias")}
    p64 = {k: getattr(conv, k).detach().double().requires_grad_(True) for k in names}
    x64 = x0.double().requires_grad_(True)
    ref = rgcn_forward(x64, ei, et, relu=relu, aggr=aggr, **{**none, **p64})[self_rows]
    (ref * G.double()).sum().backward()
    # the scale of a gradient: the same chain with every factor's magnitude
    pa = {k: v.detach().abs().requires_grad_(True) for k, v in p64.items()}
    xa = x0.double().abs().requires_grad_(True)
    mask = (runs[0][-1] > 0).double() if relu else 1.0
    ra = rgcn_forward(xa, ei, et, aggr=aggr, **{**none, **pa})[self_rows]
    (ra * (G.double().abs() * mask)).sum().backward()
    for k, got in zip(names, runs[0]):
        _close(got, p64[k].grad, pa[k].grad, "d" + k)
    if ids is None:
        _close(runs[0][-2], x64.grad, xa.grad, "dx")


@pytest.mark.parametrize("F,N,R,bases", [(32, 32, 535, 30), (64, 16, 3, None)])
def test_edge_index_and_csr_pair_paths(hiplib, F, N, R, bases):
    """(c) the ``for batch in loader`` call shape: COO edge_index with duplicates, loops and a hub row of 3000 in-edges (the
    coefficient kernel's multi-block count), int64 relation ids; the [row_ptr, col] CSR pair gives the same rows."""
    import torch
    n = 2000
    g = torch.Generator(device="cuda").manual_seed(F + R)
    E = 20000
    ei = torch.stack([torch.randint(0, n, (E,), generator=g, device="cuda"), torch.randint(0, n - 50, (E,), generator=g, device="cuda")])
    ei[1, :3000] = 7                               # a hub destination
    ei[1, 3000:3300] = ei[0, 3000:3300]            # self loops
    ei = torch.cat([ei, ei[:, 5000:5500]], 1)      # duplicate edges
    et = torch.randint(0, R, (ei.shape[1],), generator=g, device="cuda")
    et[:3000] = torch.randint(0, 3, (3000,), generator=g, device="cuda")   # many edges of the hub share a relation
    conv = _conv(F, N, R, bases, seed=4)
    x = torch.randn((n, F), device="cuda")
    with torch.no_grad():
        got = conv(x, ei, et)
    ref = rgcn_forward(x.double(), ei, et, **_params(conv))
    scale = rgcn_forward(x.double(), ei, et, abs_terms=True, **_params(conv))
    assert got.shape == (n, N)
    _close(got, ref, scale, "edge_index")
    order = torch.sort(ei[1], stable=True).indices
    rp = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    rp[1:] = torch.cumsum(torch.bincount(ei[1], minlength=n), 0)
    with torch.no_grad():
        got2 = conv(x, [rp, ei[0][order].to(torch.int32).contiguous()], et[order].to(torch.int32))
    _close(got2, ref, scale, "csr pair")
    # a destination-sorted edge_index with the loader's marker: taken in its own order, the same rows as the unsorted list
    ei_s = ei[:, order].contiguous()
    ei_s._wgamd_dst_sorted = ei_s._version
    with torch.no_grad():
        got3 = conv(x, ei_s, et[order])
    assert torch.equal(got3, got)
    xg = x.clone().requires_grad_(True)
    conv(xg, ei, et).sum().backward()
    xr = x.double().requires_grad_(True)
    rgcn_forward(xr, ei, et, **_params(conv)).sum().backward()
    assert float((xg.grad.double() - xr.grad).abs().max()) <= 1e-5 * max(1.0, float(xr.grad.abs().max()))


def test_bad_relation_ids_and_capture_refused(hiplib):
    import torch
    from wholegraph_amd import nn
    rp, col, self_rows, et = _hop(100, 300, 5, 3, seed=1)
    conv = _conv(16, 8, 3, None, seed=0)
    x = torch.randn(300, 16, device="cuda")
    lg = nn.LayerGraph([nn.HopGraph(rp, col, self_rows)])
    bad = et.clone()
    bad[-1] = 3
    with pytest.raises(ValueError, match="outside"):
        conv(x, lg, bad)
    bad[-1] = -1
    with pytest.raises(ValueError, match="outside"):
        conv(x, lg, bad)
    with pytest.raises(ValueError, match="entries"):
        conv(x, lg, et[:-1])
    with pytest.raises(ValueError, match="int32 or int64"):
        conv(x, lg, et.float())
    ei = _edge_index(rp, self_rows, col)
    with pytest.raises(ValueError, match="entries"):
        conv(x, ei, et[1:])
    table = torch.randn(500, 16, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError):
        conv(nn.LazyRows(table, torch.arange(300, device="cuda")), lg, et)
    import wholegraph_amd.nn as wnn
    orig = wnn._capturing
    wnn._capturing = lambda: True
    try:
        with pytest.raises(RuntimeError, match="capture"):
            conv(x, lg, et)
    finally:
        wnn._capturing = orig


def test_edge_type_device_length_and_fresh_coefficients(hiplib):
    """Relation ids on another device are refused on every path (the kernels never read a host pointer); a hand-built layer
    graph takes exactly its edges' count; a new relation tensor on the same layer graph gives new coefficients."""
    import torch
    from wholegraph_amd import nn
    rp, col, self_rows, et = _hop(200, 400, 8, 5, seed=3)
    conv = _conv(16, 8, 5, None, seed=0)
    x = torch.randn(400, 16, device="cuda")
    lg = nn.LayerGraph([nn.HopGraph(rp, col, self_rows)])
    with pytest.raises(ValueError, match="device|cpu"):
        conv(x, lg, et.cpu())
    n_dst = rp.shape[0] - 1
    with pytest.raises(ValueError, match="device|cpu"):
        conv(x[:n_dst].contiguous(), [rp, col.clamp(max=n_dst - 1)], et.cpu())
    ei = _edge_index(rp, self_rows, col)
    with pytest.raises(ValueError, match="device|cpu"):
        conv(x, ei, et.cpu())
    with pytest.raises(ValueError, match="entries"):
        conv(x, lg, torch.cat([et, et[:3]]))
    ref = lambda t: rgcn_forward(x.double(), ei, t, **_params(conv))[self_rows]            # noqa: E731
    scale = lambda t: rgcn_forward(x.double(), ei, t, abs_terms=True, **_params(conv))[self_rows]   # noqa: E731
    with torch.no_grad():
        for k in range(3):                         # same length, same layer graph, new values (a freed address may be reused)
            t = (et + k) % 5
            _close(conv(x, lg, t), ref(t), scale(t), "fresh coefficients %d" % k)
            del t


def test_long_rows_sort_count(hiplib):
    """COO rows above the long-row bound count relations by a sort: a hub of 10000 in-edges (mean and add) equals the
    restatement, forward and input gradient."""
    import torch
    n, R = 3000, 6
    g = torch.Generator(device="cuda").manual_seed(11)
    E = 30000
    ei = torch.stack([torch.randint(0, n, (E,), generator=g, device="cuda"), torch.randint(0, n, (E,), generator=g, device="cuda")])
    ei[1, :10000] = 17
    et = torch.randint(0, R, (E,), generator=g, device="cuda", dtype=torch.int32)
    for aggr in ("mean", "add"):
        conv = _conv(32, 16, R, 4, seed=5, aggr=aggr)
        x = torch.randn((n, 32), device="cuda", requires_grad=True)
        got = conv(x, ei, et)
        _close(got.detach(), rgcn_forward(x.detach().double(), ei, et, aggr=aggr, **_params(conv)),
               rgcn_forward(x.detach().double(), ei, et, aggr=aggr, abs_terms=True, **_params(conv)), "long rows " + aggr)
        got.sum().backward()
        xr = x.detach().double().requires_grad_(True)
        rgcn_forward(xr, ei, et, aggr=aggr, **_params(conv)).sum().backward()
        assert float((x.grad.double() - xr.grad).abs().max()) <= 1e-5 * max(1.0, float(xr.grad.abs().max()))


def _stores(V, F, R, seed):
    """A power-law graph with self loops and duplicated edges, features and a relation id per edge on the device."""
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
    rel = torch.from_numpy(rng.integers(0, R, src_all.shape[0])).cuda()
    fs[("n", "e", "n"), "rel", None] = rel
    return gs, fs, rel


@pytest.mark.parametrize("fanout", [[10, 5], [15, 10, 5]])
def test_call_group_rgcn_equals_per_batch_fp64(hiplib, fanout):
    """(d) a 2-layer RGCN over a call group's trimmed layer graphs (lazy x, edge_type = cg.edge_attr("rel") for both layers)
    equals, at every seed, the float64 restatement run on each mini-batch of ``to_data_list()`` with ``rel[batch.e_id]``;
    ``edge_attr`` equals the feature store read through ``e_id``."""
    import torch
    from cugraph_pyg_amd.loader import NeighborLoader
    V, F0, R = 6000, 32, 12
    gs, fs, rel = _stores(V, F0, R, seed=23)
    H = len(fanout)
    dims = [F0] + [32] * (H - 1) + [8]
    convs = [_conv(dims[i], dims[i + 1], R, 4 if i % 2 == 0 else None, seed=30 + i) for i in range(H)]
    B, G = 48, 3
    seeds = torch.randperm(V, generator=torch.Generator().manual_seed(2))[:G * B].cuda()
    loader = NeighborLoader((fs, gs), fanout, input_nodes=seeds, batch_size=B, shuffle=False, random_state=7,
                            local_seeds_per_call=G * B)
    grp = next(iter(loader.call_groups()))
    et = grp.edge_attr("rel")
    assert torch.equal(et, fs[("n", "e", "n"), "rel", None][grp.e_id])
    with torch.no_grad():
        h = grp.x
        for j, c in enumerate(convs):
            h = c(h, grp.layer_graph(j), et, act="relu" if j + 1 < H else None)
    refs, scales = [], []
    for d in grp.to_data_list():
        r, s = d.x.double().cuda(), d.x.double().cuda()
        ed = rel[d.e_id.cuda()]
        for j, c in enumerate(convs):
            r = rgcn_forward(r, d.edge_index, ed, relu=j + 1 < H, **_params(c))
            s = rgcn_forward(s, d.edge_index, ed, abs_terms=True, **_params(c))
        refs.append(r[:d.batch_size])
        scales.append(s[:d.batch_size])
    ref, scale = torch.cat(refs), torch.cat(scales)
    assert h.shape == ref.shape
    _close(h, ref, scale, "logits")


def test_link_loader_loop_forward_backward(hiplib):
    """(e) the reference example's loop: ``for batch in LinkNeighborLoader(...)`` with ``conv(x, batch.edge_index,
    rel[batch.e_id])`` and a trainable embedding — forward and backward, gradients finite, matching the float64 forward."""
    import torch
    from cugraph_pyg_amd.loader import LinkNeighborLoader
    V, R = 3000, 7
    gs, fs, rel = _stores(V, 8, R, seed=5)
    emb = torch.nn.Parameter(torch.randn(V, 32, device="cuda"))
    convs = [_conv(32, 32, R, 30, seed=40), _conv(32, 32, R, 30, seed=41)]
    src = torch.randint(0, V, (400,), generator=torch.Generator().manual_seed(3)).cuda()
    dst = torch.randint(0, V, (400,), generator=torch.Generator().manual_seed(4)).cuda()
    loader = LinkNeighborLoader((fs, gs), [10, 5], edge_label_index=torch.stack([src, dst]), batch_size=200, random_state=3)
    n = 0
    for batch in loader:
        x = emb[batch.n_id.cuda()]
        et = rel[batch.e_id.cuda()]
        h = convs[0](x, batch.edge_index, et, act="relu")
        h = convs[1](h, batch.edge_index, et)
        with torch.no_grad():
            r = rgcn_forward(x.double(), batch.edge_index, et, relu=True, **_params(convs[0]))
            r = rgcn_forward(r, batch.edge_index, et, **_params(convs[1]))
        assert float((h.detach().double() - r).abs().max()) <= 1e-4 * max(1.0, float(r.abs().max()))
        h.square().mean().backward()
        n += 1
    assert n == 2
    assert emb.grad is not None and bool(torch.isfinite(emb.grad).all()) and float(emb.grad.abs().sum()) > 0
    for c in convs:
        for p in c.parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all())
