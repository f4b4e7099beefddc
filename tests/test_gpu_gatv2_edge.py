"""GPU parity of wholegraph_amd.nn.GATv2EdgeConv (csrc/wg_gatv2_edge.hip) against the float64 restatement of PyG's
GATv2Conv(edge_dim) (tests/gatv2_edge_ref.py) at the bars of test_gpu_transformer.py — ``_close`` (|err| <= 1e-5 x the magnitude sum
of the terms + 1e-7; the message has GATv2Conv's terms), alpha to 1e-5, ``_close_grad`` (max |err| <= 1e-4 max |ref|) — over the hop
of test_gpu_gatv2.py: rows of degree 0 and 24, one row of 3000 edges, a hub source, sampled loops and duplicates, 700 = 43 x 16 + 12
rows.  Self loops (fill "mean" / a float), concat, shared weights, ReLU and the graph's form rotate through the cases."""
import pytest

from gatv2_edge_ref import edge_params_of, gatv2_edge_forward, with_loops
from test_gpu_transformer import _close, _close_grad, _edge_index, _hop

pytestmark = pytest.mark.gpu

N_DST, N_SRC = 700, 1600
# ((F, H, C, D), add_self_loops, fill_value, concat, share_weights, relu, graph form)
CASES = [((32, 4, 64, 16), True, "mean", True, False, False, "layer"),      # all lanes busy, the largest D
         ((16, 2, 12, 1), True, 0.5, False, True, True, "csr"),             # lanes per head no power of two, D = 1
         ((16, 8, 8, 6), False, "mean", True, False, True, "coo"),          # D no multiple of 4
         ((16, 1, 16, 17), True, "mean", False, True, False, "layer")]      # outside the kernel domain: the torch route


def _conv(F, H, C, D, seed, **kw):
    import torch
    from wholegraph_amd import nn
    torch.manual_seed(seed)
    conv = nn.GATv2EdgeConv(F, C, D, heads=H, **kw).cuda()
    with torch.no_grad():
        conv.att.mul_(3.0)                                     # logits of order 1-10: a softmax neither flat nor one-hot
        for b in (conv.lin_l.bias, conv.lin_r.bias, conv.bias):
            b.uniform_(-0.5, 0.5)
    return conv


@pytest.fixture
def launches(monkeypatch):
    """Counts the one-launch forwards (``gatv2_edge_attention`` calls) of the test."""
    import wholegraph_amd.nn as wnn
    calls, orig = [], wnn.gatv2_edge_attention
    monkeypatch.setattr(wnn, "gatv2_edge_attention", lambda *a, **kw: calls.append(1) or orig(*a, **kw))
    return calls


@pytest.mark.parametrize("case", range(len(CASES)))
def test_layer_vs_fp64(hiplib, launches, case):
    """Forward, alpha and the gradients of x, lin_l, lin_r, lin_edge, att and bias over one hop; the backward twice with the same
    bits; the destination-major backward over 3 workgroups (44 tiles at a fixed stride) sums to the same dW_e."""
    import torch
    from wholegraph_amd import nn
    (F, H, C, D), loops, fill, concat, share, relu, form = CASES[case]
    inside = D <= 16
    rp, col, self_rows = _hop(N_DST, N_SRC, 24, seed=case, hub=3000)
    if form != "layer":                                        # COO and CSR pairs: the destinations are the first rows of x
        self_rows = torch.arange(N_DST, device="cuda")
    conv = _conv(F, H, C, D, seed=case, concat=concat, share_weights=share, add_self_loops=loops, fill_value=fill)
    assert nn.gatv2_edge_supported(H, C, D) == inside and conv.route == ("kernel" if inside else "torch")
    x0 = torch.randn((N_SRC, F), device="cuda")
    ea = torch.randn((col.shape[0], D), device="cuda")
    ei = _edge_index(rp, self_rows, col)
    G = torch.randn((N_DST, H * C if concat else C), device="cuda")
    if form == "coo":                                          # destinations backwards, a row's edges in their order
        order = torch.sort(-ei[1], stable=True).indices
        graph, ea_in = ei[:, order].contiguous(), ea[order]
    else:
        graph, ea_in = ([rp, col], ea) if form == "csr" else (nn.LayerGraph([nn.HopGraph(rp, col, self_rows)]), ea)
    runs = []
    for _ in range(2):
        conv.zero_grad(set_to_none=True)
        xs = x0.clone().requires_grad_(True)
        out = conv((xs, xs[:N_DST]) if form == "coo" else xs, graph, act="relu" if relu else None, edge_attr=ea_in)
        (out * G).sum().backward()
        runs.append(dict({k: p.grad.clone() for k, p in conv.named_parameters()}, x=xs.grad.clone(), out=out.detach().clone()))
    assert len(launches) == (2 if inside else 0)
    for k in runs[0] if inside else []:                        # (the kernels'; the torch route adds with index_add)
        assert torch.equal(runs[0][k], runs[1][k]), "not run-to-run deterministic: " + k
    p64 = {k: v.double().requires_grad_(True) for k, v in edge_params_of(conv).items()}
    if share:
        p64["Wr"], p64["br"] = p64["Wl"], p64["bl"]
    x64 = x0.double().requires_grad_(True)
    ei2, rows2 = with_loops(ei, ea, self_rows, fill) if loops else (ei, ea.double())
    ref, ra = gatv2_edge_forward(x64, ei2, rows2, p64, H, concat, relu=relu, return_alpha=True)
    scale = gatv2_edge_forward(x64.detach(), ei2, rows2, {k: v.detach() for k, v in p64.items()}, H, concat, abs_terms=True)
    (ref[self_rows] * G.double()).sum().backward()
    got = runs[0]
    _close(got["out"], ref.detach()[self_rows], scale[self_rows], "forward")
    names = {"lin_l.weight": "Wl", "lin_l.bias": "bl", "lin_edge.weight": "We", "att": "att", "bias": "bias"}
    if not share:
        names.update({"lin_r.weight": "Wr", "lin_r.bias": "br"})
    assert sorted(got) == sorted(list(names) + ["x", "out"])
    for k, r in names.items():
        _close_grad(got[k], p64[r].grad, "d" + k)
    _close_grad(got["x"], x64.grad, "dx")
    if not inside:
        return
    # the launches on their own, on the layer's XL / XR and the rows of the CSR the kernels walk
    hop = nn.HopGraph(rp, col, self_rows)
    rp2, col2 = hop.with_self_loops() if loops else (rp, col)
    with torch.no_grad():
        XL = conv.lin_l(x0)
        XR, rows = (XL, self_rows) if share else (conv.lin_r(x0[self_rows]), None)
        ea2 = nn._gatv2_edge_rows(hop, ea, conv._fill_rows(hop, ea)) if loops else ea
        wet = conv.lin_edge.weight.t().contiguous()
        out2, alpha, agg = nn.gatv2_edge_attention(rp2, col2, XL, XR, conv.att, H, ea2, wet, xr_rows=rows, bias=conv.bias, relu=relu,
                                                   need_alpha=True, mean=not concat)
        assert torch.equal(out2, got["out"])
        # (the restatement lists all loops first; the kernel's CSR has each in front of its row: edge k of row i at slot k + i + 1)
        at = torch.arange(col.shape[0], device="cuda")
        if loops:
            at = torch.cat([rp2[:N_DST].long(), at + torch.repeat_interleave(torch.arange(N_DST, device="cuda"), (rp[1:] - rp[:-1]).long()) + 1])
        assert float((alpha[at].double() - ra.detach()).abs().max()) <= 1e-5, "alpha"
        Gf = G * (got["out"] > 0) if relu else G                  # dL/d agg, as the layer's backward forms it
        Gf = Gf if concat else (Gf * (1.0 / H)).repeat(1, H)
        few = nn.gatv2_edge_bwd_dst(rp2, col2, XL, XR, conv.att, H, ea2, wet, alpha, Gf.contiguous(), agg, xr_rows=rows, max_blocks=3)
    assert few[3].shape == (3, D, H * C)
    _close_grad(few[3].sum(0).t(), p64["We"].grad, "dW_e over 3 workgroups")


def test_two_hop_layer_graph_reads_prefixes_of_one_edge_attr(hiplib, launches):
    """Two layers over a two-hop / one-hop LayerGraph pair take the SAME hop-major edge_attr: each hop equals the layer run on that
    hop alone with its slice; an empty hop makes no launch."""
    import torch
    from wholegraph_amd import nn
    F, H, C, D = 16, 4, 8, 5
    rp1, col1, s1 = _hop(N_DST, N_SRC, 24, seed=7, hub=3000)
    rp2, col2, s2 = _hop(300, N_SRC, 9, seed=8)
    h1, h2 = nn.HopGraph(rp1, col1, s1), nn.HopGraph(rp2, col2, s2)
    none = nn.HopGraph(torch.zeros(1, dtype=torch.int32, device="cuda"), col1[:0], s1[:0])
    E1, E2 = col1.shape[0], col2.shape[0]
    ea = torch.randn((E1 + E2, D), device="cuda")
    conv = _conv(F, H, C, D, seed=9)
    x = torch.randn((N_SRC, F), device="cuda")
    two, one = nn.LayerGraph([h1, none, h2]), nn.LayerGraph([h1])
    two.num_group_edges = one.num_group_edges = E1 + E2
    with torch.no_grad():
        both, first = conv(x, two, act="relu", edge_attr=ea), conv(x, one, act="relu", edge_attr=ea)
        assert len(launches) == 3
        alone = conv(x, nn.LayerGraph([h2]), act="relu", edge_attr=ea[E1:])
    assert torch.equal(both[:N_DST], first) and torch.equal(both[N_DST:], alone)
    with pytest.raises(ValueError, match="rows for"):
        conv(x, one, edge_attr=ea[:E1])
