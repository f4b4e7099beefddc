"""GPU parity of wholegraph_amd.nn.GATv2Conv (csrc/wg_gatv2.hip): the one-launch attention per hop, the kernel on its own, every
gradient (x, lin_l, lin_r, att, bias) with its bit-reproducibility, the three graph forms and the call-group route, against the
float64 restatement of torch_geometric.nn.GATv2Conv (tests/gatv2_ref.py) at the project's bars — ``_close`` (|err| <= 1e-5 x the
magnitude sum of the terms + 1e-7) and ``_close_grad`` (max |err| <= 1e-4 max |ref|) of test_gpu_transformer.py, over hops built
by its ``_hop``: rows of degree 0 and 24, one row of 3000 edges (many rescales of the online softmax), 10 % of the edges into
source 5 (a hub of the transposed kernel), sampled loops and duplicates, 700 = 43 x 16 + 12 rows."""
import pytest

from gatv2_ref import gatv2_forward, params_of
from test_gpu_transformer import _close, _close_grad, _edge_index, _hop, _stores

pytestmark = pytest.mark.gpu

SHAPES = [(100, 4, 64),      # all 64 lanes busy
          (64, 1, 256),      # one head across the wave
          (32, 8, 8),        # two lanes per head, 48 idle
          (48, 2, 12),       # three lanes per head: not a power of two
          (16, 3, 16)]
OUTSIDE = (64, 1, 47)
N_DST, N_SRC = 700, 1600


def _conv(F, C, H, seed, **kw):
    import torch
    from wholegraph_amd import nn
    torch.manual_seed(seed)
    conv = nn.GATv2Conv(F, C, heads=H, **kw).cuda()
    with torch.no_grad():
        conv.att.mul_(3.0)                                     # logits of order 1-10: a softmax neither flat nor one-hot
        for b in (conv.lin_l.bias, conv.lin_r.bias, conv.bias):
            b.uniform_(-0.5, 0.5)
    return conv


@pytest.fixture
def launches(monkeypatch):
    """Counts the one-launch forwards (``gatv2_attention`` calls) of the test."""
    import wholegraph_amd.nn as wnn
    calls, orig = [], wnn.gatv2_attention

    def counted(*a, **kw):
        calls.append(1)
        return orig(*a, **kw)
    monkeypatch.setattr(wnn, "gatv2_attention", counted)
    return calls


def _kernel_edges(hop, loops):
    """``(row_ptr, col, edge_index)`` of the CSR the kernel walks — the self loop first in every row — with the edge list in
    the same order (destinations as input rows)."""
    rp, col = hop.with_self_loops() if loops else (hop.row_ptr, hop.col)
    return rp, col, _edge_index(rp, hop.self_rows, col)


# ((F, H, C), add_self_loops, concat, share_weights, relu, lazy ids)
FWD = [(SHAPES[0], True, True, False, False, None),
       (SHAPES[1], False, False, True, True, "int32"),
       (SHAPES[2], True, False, False, True, "int64"),
       (SHAPES[3], False, True, True, False, None),
       (SHAPES[4], True, True, True, True, "int32"),
       (OUTSIDE, True, False, False, False, "int64"),
       (SHAPES[0], False, False, True, True, "int64"),
       (SHAPES[2], True, True, True, False, None),
       (SHAPES[3], True, False, False, True, "int32")]


@pytest.mark.parametrize("case", range(len(FWD)))
def test_layer_forward_vs_fp64(hiplib, launches, case):
    """(1) the layer over one hop; self loops, concat, shared weights, relu and the form of x (tensor, LazyRows with int32 / int64
    ids) rotate through the cases.  Inside the domain exactly ONE launch and route "kernel"; outside none and "torch".  alpha
    (need_alpha of the launch, on the layer's own XL / XR) against the restatement's to 1e-5."""
    import torch
    from wholegraph_amd import nn
    (F, H, C), loops, concat, share, relu, ids = FWD[case]
    inside = (F, H, C) != OUTSIDE
    rp, col, self_rows = _hop(N_DST, N_SRC, 24, seed=case, hub=3000)
    conv = _conv(F, C, H, seed=case, concat=concat, share_weights=share, add_self_loops=loops)
    assert nn.gatv2_supported(H, C) == inside and conv.route == ("kernel" if inside else "torch")
    table = torch.randn((3000, F), device="cuda")
    if ids is None:
        x, xd = table[:N_SRC].contiguous(), table[:N_SRC]
    else:
        idv = torch.randperm(3000, device="cuda")[:N_SRC].to(getattr(torch, ids))
        x, xd = nn.LazyRows(table, idv), table[idv.long()]
    hop = nn.HopGraph(rp, col, self_rows)
    with torch.no_grad():
        got = conv(x, nn.LayerGraph([hop]), act="relu" if relu else None)
    assert len(launches) == (1 if inside else 0)
    rp2, col2, ei = _kernel_edges(hop, loops)
    p = params_of(conv)
    ref, ra = gatv2_forward(xd, None, ei, p, H, concat, relu=relu, return_alpha=True)
    scale = gatv2_forward(xd, None, ei, p, H, concat, abs_terms=True)
    assert got.shape == (N_DST, H * C if concat else C)
    _close(got, ref[self_rows], scale[self_rows], "forward")
    if inside:
        with torch.no_grad():
            XL = conv.lin_l(xd)
            XR, rows = (XL, self_rows) if share else (conv.lin_r(xd[self_rows]), None)
            out2, alpha, agg = nn.gatv2_attention(rp2, col2, XL, XR, conv.att, H, xr_rows=rows, bias=conv.bias, relu=relu,
                                                  need_alpha=True, mean=not concat)
        assert torch.equal(out2, got) and alpha.shape == (col2.shape[0], H) and agg.shape == (N_DST, H * C)
        assert float((alpha.double() - ra).abs().max()) <= 1e-5, "alpha"


@pytest.mark.parametrize("H,C", [(4, 64), (2, 12), (8, 8)])
@pytest.mark.parametrize("by_rows", [False, True])
def test_kernel_alone_vs_fp64(hiplib, H, C, by_rows):
    """(2) ``nn.gatv2_attention`` on given float32 XL, XR, att — XR dense, or read at ``xr_rows`` — against the restatement on
    the same float32 values (identity weights), no self loops: rows 0 and 3 have no entry and come out as the bias exactly."""
    import torch
    from wholegraph_amd import nn
    HC = H * C
    rp, col, self_rows = _hop(N_DST, N_SRC, 24, seed=H + C, hub=3000)
    g = torch.Generator(device="cuda").manual_seed(C)
    XL = torch.randn((N_SRC, HC), generator=g, device="cuda")
    XRd = XL[self_rows].contiguous() if by_rows else torch.randn((N_DST, HC), generator=g, device="cuda")
    att = torch.randn((1, H, C), generator=g, device="cuda") * (3.0 / C ** 0.5)
    bias = torch.rand(HC, generator=g, device="cuda") - 0.5
    eye = torch.eye(HC, dtype=torch.float64, device="cuda")
    ei = _edge_index(rp, torch.arange(N_DST, device="cuda"), col)
    for mean, relu in [(False, False), (True, True)]:
        b = bias[:C].contiguous() if mean else bias
        p = dict(Wl=eye, bl=None, Wr=eye, br=None, att=att, bias=b)
        out, alpha, agg = nn.gatv2_attention(rp, col, XL, XL if by_rows else XRd, att, H, xr_rows=self_rows if by_rows else None,
                                             bias=b, relu=relu, need_alpha=True, mean=mean)
        ref, ra = gatv2_forward(XL, XRd, ei, p, H, not mean, relu=relu, return_alpha=True)
        scale = gatv2_forward(XL, XRd, ei, p, H, not mean, abs_terms=True)
        _close(out, ref, scale, "kernel")
        assert float((alpha.double() - ra).abs().max()) <= 1e-5
        want = torch.relu(b) if relu else b
        assert torch.equal(out[0], want) and torch.equal(out[3], want), "a row without entries: zeros plus bias"
        assert not bool(agg[0].any()) and not bool(agg[3].any())
        plain = nn.gatv2_attention(rp, col, XL, XL if by_rows else XRd, att, H, xr_rows=self_rows if by_rows else None, bias=b,
                                   relu=relu, mean=mean)
        assert torch.equal(plain, out), "need_alpha changes no bit of the output"


def test_empty_hops(hiplib):
    """(2) no rows, and rows without any entry: no launch, zeros plus bias."""
    import torch
    from wholegraph_amd import nn
    H, C = 2, 8
    XL = torch.randn((10, H * C), device="cuda")
    att, bias = torch.randn((1, H, C), device="cuda"), torch.randn(H * C, device="cuda")
    none = torch.zeros(0, dtype=torch.int32, device="cuda")
    out = nn.gatv2_attention(torch.zeros(1, dtype=torch.int32, device="cuda"), none, XL, XL[:0], att, H, bias=bias)
    assert out.shape == (0, H * C)
    out, alpha, agg = nn.gatv2_attention(torch.zeros(6, dtype=torch.int32, device="cuda"), none, XL, XL[:5], att, H, bias=bias,
                                         need_alpha=True)
    assert torch.equal(out, bias.expand(5, -1)) and alpha.shape == (0, H) and not bool(agg.any())
    conv = _conv(16, C, H, seed=0, add_self_loops=False)
    lg = nn.LayerGraph([nn.HopGraph(torch.zeros(6, dtype=torch.int32, device="cuda"), none, torch.arange(5, device="cuda")),
                        nn.HopGraph(torch.zeros(1, dtype=torch.int32, device="cuda"), none, torch.arange(0, device="cuda"))])
    x = torch.randn((10, 16), device="cuda", requires_grad=True)
    out = conv(x, lg, act="relu")
    assert torch.equal(out.detach(), torch.relu(conv.bias.detach()).expand(5, -1))
    out.sum().backward()
    assert not bool(x.grad.any()) and not bool(conv.att.grad.any()) and bool(torch.isfinite(conv.bias.grad).all())


BWD = [(s, share, concat) for s in (SHAPES[0], SHAPES[2], SHAPES[3]) for share in (False, True) for concat in (True, False)]


@pytest.mark.parametrize("case", range(len(BWD)))
def test_layer_backward_vs_fp64_and_deterministic(hiplib, launches, case):
    """(3) the gradients of x, lin_l, lin_r, att and bias against float64 autograd of the restatement; two backward passes on
    the same inputs give the same bits.  Self loops and relu alternate through the cases."""
    import torch
    from wholegraph_amd import nn
    (F, H, C), share, concat = BWD[case]
    loops, relu = case % 2 == 0, case % 3 == 0
    rp, col, self_rows = _hop(N_DST, N_SRC, 24, seed=10 + case, hub=3000)
    conv = _conv(F, C, H, seed=20 + case, concat=concat, share_weights=share, add_self_loops=loops)
    N = H * C if concat else C
    x0 = torch.randn((N_SRC, F), device="cuda")
    G = torch.randn((N_DST, N), device="cuda")
    hop = nn.HopGraph(rp, col, self_rows)
    lg = nn.LayerGraph([hop])
    runs = []
    for _ in range(2):
        conv.zero_grad(set_to_none=True)
        xs = x0.clone().requires_grad_(True)
        out = conv(xs, lg, act="relu" if relu else None)
        (out * G).sum().backward()
        grads = {k: p.grad.clone() for k, p in conv.named_parameters()}
        grads["x"] = xs.grad.clone()
        runs.append((out.detach().clone(), grads))
    assert len(launches) == 2, "the kernel route: one forward launch per hop"
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), "backward is not run-to-run deterministic: " + k
    p64 = {k: v.double().requires_grad_(True) for k, v in params_of(conv).items()}
    if share:
        p64["Wr"], p64["br"] = p64["Wl"], p64["bl"]
    x64 = x0.double().requires_grad_(True)
    ei = _kernel_edges(hop, loops)[2]
    ref = gatv2_forward(x64, None, ei, p64, H, concat, relu=relu)[self_rows]
    (ref * G.double()).sum().backward()
    got = runs[0][1]
    names = {"lin_l.weight": "Wl", "lin_l.bias": "bl", "att": "att", "bias": "bias"}
    if not share:
        names.update({"lin_r.weight": "Wr", "lin_r.bias": "br"})
    assert sorted(got) == sorted(list(names) + ["x"])
    for k, r in names.items():
        _close_grad(got[k], p64[r].grad, "d" + k)
    _close_grad(got["x"], x64.grad, "dx")


@pytest.mark.parametrize("loops,concat,share", [(True, True, False), (False, False, True), (True, False, True)])
def test_graph_forms_agree(hiplib, launches, loops, concat, share):
    """(4) COO (the sampler-layout pair), the CSR pair and a one-hop LayerGraph with self_rows = arange give the same bits; a
    two-hop LayerGraph equals the per-hop results back to back, one launch per hop."""
    import torch
    from wholegraph_amd import nn
    F, H, C = 32, 4, 16
    rp, col, _ = _hop(N_DST, N_SRC, 24, seed=3, hub=3000)
    conv = _conv(F, C, H, seed=4, concat=concat, share_weights=share, add_self_loops=loops)
    x = torch.randn((N_SRC, F), device="cuda")
    ar = torch.arange(N_DST, device="cuda")
    ei = _edge_index(rp, ar, col)
    ei = ei[:, torch.sort(-ei[1], stable=True).indices].contiguous()       # destinations backwards, a row's edges in their order
    with torch.no_grad():
        a = conv((x, x[:N_DST]), ei)
        b = conv(x, [rp, col])
        c = conv(x, nn.LayerGraph([nn.HopGraph(rp, col, ar)]))
    assert len(launches) == 3
    assert a.shape == (N_DST, H * C if concat else C) and torch.equal(a, b) and torch.equal(b, c)
    rp2, col2, self2 = _hop(300, N_SRC, 9, seed=5)
    _, _, self1 = _hop(N_DST, N_SRC, 24, seed=3, hub=3000)
    h1, h2 = nn.HopGraph(rp, col, self1), nn.HopGraph(rp2, col2, self2)
    del launches[:]
    with torch.no_grad():
        both = conv(x, nn.LayerGraph([h1, h2]), act="relu")
        assert len(launches) == 2
        one, two = conv(x, nn.LayerGraph([h1]), act="relu"), conv(x, nn.LayerGraph([h2]), act="relu")
    assert both.shape[0] == N_DST + 300 and torch.equal(both, torch.cat([one, two]))


def test_call_group_route(hiplib, launches):
    """(5) two GATv2Conv layers over a call group's trimmed layer graphs: a lazy x equals the dense x bit for bit, and the
    seeds' outputs match the float64 per-batch formulation over ``to_data_list()`` (a self loop at every node) at 1e-5 max |ref|,
    the bar of test_gpu_temporal_call_groups.py for the same comparison.  A HeteroLayerGraph is refused."""
    import torch
    from cugraph_pyg_amd.loader import NeighborLoader
    from wholegraph_amd import nn
    V, F0 = 6000, 32
    gs, fs, _ = _stores(V, F0, 1, seed=23)
    convs = [_conv(F0, 16, 4, seed=30, concat=True), _conv(64, 8, 1, seed=31, concat=False, share_weights=True)]
    B, G = 96, 3
    seeds = torch.randperm(V, generator=torch.Generator().manual_seed(2))[:G * B].cuda()
    loader = NeighborLoader((fs, gs), [10, 5], input_nodes=seeds, batch_size=B, shuffle=False, random_state=7,
                            local_seeds_per_call=G * B)
    grp = next(iter(loader.call_groups()))

    def forward(h):
        with torch.no_grad():
            for j, c in enumerate(convs):
                h = c(h, grp.layer_graph(j), act="relu" if j == 0 else None)
        return h
    lazy = forward(grp.x)
    assert isinstance(grp.x, nn.LazyRows)
    assert len(launches) == len(grp.layer_graph(0).hops) + len(grp.layer_graph(1).hops) == 3
    dense = forward(grp.node_attr("x", lazy=False))
    assert lazy.shape == (grp.num_seeds, 8) and torch.equal(lazy, dense)
    refs = []
    for d in grp.to_data_list():
        r = d.x.double().cuda()
        ar = torch.arange(r.shape[0], device="cuda")
        ei = torch.cat([torch.stack([ar, ar]), torch.as_tensor(d.edge_index).cuda()], 1)
        for j, c in enumerate(convs):
            r = gatv2_forward(r, None, ei, params_of(c), c.heads, c.concat, relu=j == 0)
        refs.append(r[:d.batch_size])
    ref = torch.cat(refs)
    assert lazy.shape == ref.shape
    err = float((lazy.double() - ref).abs().max())
    assert err <= 1e-5 * float(ref.abs().max()), (err, float(ref.abs().max()))
    with pytest.raises(NotImplementedError, match="heterogeneous"):
        convs[0](grp.x, nn.HeteroLayerGraph([], {}, []))
