"""GPU parity of wholegraph_amd.nn.GINEConv (csrc/wg_gine.hip) against the float64 restatement of PyG's GINEConv
(tests/gine_ref.py) at the bars of test_gpu_transformer.py — ``_close`` (|err| <= 1e-5 x the magnitude sum of the terms + 1e-7),
``_close_grad`` (max |err| <= 1e-4 max |ref|) — over its hop: rows of degree 0 and 24 (across the eight-edge unroll), one row of
3000 edges, a hub source (the 64-entry pieces of the source-major kernel), sampled loops and duplicates, 700 = 43 x 16 + 12 rows.
The graph's form, the trailing ReLU, train_eps and a LazyRows input rotate through the cases."""
import pytest

from gine_ref import gine_forward, params_of
from test_gpu_transformer import _close, _close_grad, _edge_index, _hop

pytestmark = pytest.mark.gpu

N_DST, N_SRC = 700, 1600
# ((F, H, N, D), graph form, relu, train_eps, lazy)
CASES = [((256, 256, 256, 16), "layer", False, True, False),     # all lanes busy, the largest D, the LDS maximum
         ((20, 36, 12, 3), "csr", True, False, False),           # F, H no multiples of 16, D no multiple of 4, half-filled mask words
         ((4, 4, 4, 1), "coo", False, True, False),              # one float4 per row, the smallest lane group
         ((32, 64, 0, 5), "layer", True, False, True),           # the "linear" route through the one-product form
         ((48, 16, 8, None), "csr", False, True, False),         # edge rows of width F, no lin
         ((16, 8, 8, 17), "coo", True, False, False)]            # outside the domain: the torch route, the same bars


def _conv(F, H, N, D, seed, train_eps):
    import torch
    from wholegraph_amd import nn
    torch.manual_seed(seed)
    mods = [torch.nn.Linear(F, H), torch.nn.ReLU()] + ([torch.nn.Linear(H, N)] if N else [])
    return nn.GINEConv(torch.nn.Sequential(*mods), eps=0.25, train_eps=train_eps, edge_dim=D).cuda()


@pytest.fixture
def launches(monkeypatch):
    """Counts the one-launch forwards (``gine_layer_forward`` calls) of the test."""
    import wholegraph_amd.nn as wnn
    calls, orig = [], wnn.gine_layer_forward
    monkeypatch.setattr(wnn, "gine_layer_forward", lambda *a, **kw: calls.append(1) or orig(*a, **kw))
    return calls


@pytest.mark.parametrize("case", range(len(CASES)))
def test_layer_vs_fp64(hiplib, launches, case):
    """Forward and the gradients of x, nn, lin and eps over one hop; two runs with the same bits; one forward launch per hop; the
    destination-major backward over 3 workgroups (44 tiles at a fixed stride) sums to the same d lin."""
    import torch
    from wholegraph_amd import nn
    (F, H, N, D), form, relu, train_eps, lazy = CASES[case]
    inside = D is None or D <= 16
    rp, col, self_rows = _hop(N_DST, N_SRC, 24, seed=case, hub=3000)
    if form != "layer":                                        # COO and CSR pairs: the destinations are the first rows of x
        self_rows = torch.arange(N_DST, device="cuda")
    conv = _conv(F, H, N, D, case, train_eps)
    assert nn.gine_layer_supported(F, H, N, D or 0) == inside
    assert conv.route == (("mlp" if N else "linear") if inside else "torch")
    x0 = torch.randn((N_SRC, F), device="cuda")
    ea = torch.randn((col.shape[0], D or F), device="cuda")
    ei = _edge_index(rp, self_rows, col)
    G = torch.randn((N_DST, N or H), device="cuda")
    if form == "coo":                                          # destinations backwards, a row's edges in their order
        order = torch.sort(-ei[1], stable=True).indices
        graph, ea_in = ei[:, order].contiguous(), ea[order]
    else:
        graph, ea_in = ([rp, col], ea) if form == "csr" else (nn.LayerGraph([nn.HopGraph(rp, col, self_rows)]), ea)
    ids = torch.randperm(5000, device="cuda")[:N_SRC]          # lazy: x0 = table[ids], read in the kernel through ids
    table = torch.zeros((5000, F), device="cuda")
    table[ids] = x0
    runs = []
    for _ in range(2):
        conv.zero_grad(set_to_none=True)
        xs = x0.clone().requires_grad_(True)
        xin = nn.LazyRows(table, ids) if lazy else ((xs, xs[:N_DST]) if form == "coo" else xs)
        out = conv(xin, graph, act="relu" if relu else None, edge_attr=ea_in)
        (out * G).sum().backward()
        runs.append(dict({k: p.grad.clone() for k, p in conv.named_parameters()}, out=out.detach().clone(),
                         **({} if lazy else {"x": xs.grad.clone()})))
    assert len(launches) == (2 if inside else 0)
    for k in runs[0] if inside else []:                        # (the kernels'; the torch route adds with index_add)
        assert torch.equal(runs[0][k], runs[1][k]), "not run-to-run deterministic: " + k
    p64 = {k: v.double().requires_grad_(True) for k, v in params_of(conv, [m for m in conv.nn if isinstance(m, torch.nn.Linear)]).items()}
    x64 = x0.double().requires_grad_(True)
    where = torch.zeros(N_SRC, dtype=torch.int64, device="cuda")
    where[self_rows] = torch.arange(N_DST, device="cuda")
    ei64 = torch.stack([ei[0], where[ei[1]]])                  # destinations by output row
    ref = gine_forward(x64, x64[self_rows], ei64, ea, p64, relu=relu or not N)
    scale = gine_forward(x0, x0[self_rows], ei64, ea, {k: v.detach() for k, v in p64.items()}, abs_terms=True)
    (ref * G.double()).sum().backward()
    got = runs[0]
    _close(got["out"], ref.detach(), scale, "forward")
    names = {"nn.0.weight": "W1", "nn.0.bias": "b1"}
    names.update({"nn.2.weight": "W2", "nn.2.bias": "b2"} if N else {})
    names.update({"lin.weight": "We", "lin.bias": "be"} if D else {})
    names.update({"eps": "eps"} if train_eps else {})
    assert sorted(got) == sorted(list(names) + ["out"] + ([] if lazy else ["x"]))
    for k, r in names.items():
        _close_grad(got[k], p64[r].grad.reshape(got[k].shape), "d" + k)
    if not lazy:
        _close_grad(got["x"], x64.grad, "dx")
    if not inside or not D:
        return
    # the destination-major launch on its own over 3 workgroups, on the layer's own mask bits and dAgg
    with torch.no_grad():
        lins = [m for m in conv.nn if isinstance(m, torch.nn.Linear)]
        w2, b2 = (lins[1].weight, lins[1].bias) if N else (None, None)
        out2, agg, hidden, mask = nn.gine_layer_forward(rp, col, x0, self_rows, ea, conv.lin.weight.t().contiguous(), conv.lin.bias,
                                                        lins[0].weight, lins[0].bias, w2, b2, eps=conv.eps.detach(),
                                                        relu_out=relu and bool(N), keep=True)
        assert torch.equal(out2, got["out"])
        g1 = G * (out2 > 0) if relu or not N else G
        if N:
            g1 = (g1 @ w2) * (hidden > 0)
        few = nn.gine_bwd_dst(rp, ea, mask, (g1 @ lins[0].weight).contiguous(), max_blocks=3)
    assert few.shape == (3, D + 1, F)
    _close_grad(few.sum(0)[:D].t(), p64["We"].grad, "d lin.weight over 3 workgroups")
    _close_grad(few.sum(0)[D], p64["be"].grad, "d lin.bias over 3 workgroups")


def test_two_hop_layer_graph_reads_prefixes_of_one_edge_attr(hiplib, launches):
    """Two layers over a two-hop / one-hop LayerGraph pair take the SAME hop-major edge_attr: each hop equals the layer run on that
    hop alone with its slice; an empty hop makes no launch."""
    import torch
    from wholegraph_amd import nn
    F, H, N, D = 16, 8, 8, 5
    rp1, col1, s1 = _hop(N_DST, N_SRC, 24, seed=7, hub=3000)
    rp2, col2, s2 = _hop(300, N_SRC, 9, seed=8)
    h1, h2 = nn.HopGraph(rp1, col1, s1), nn.HopGraph(rp2, col2, s2)
    none = nn.HopGraph(torch.zeros(1, dtype=torch.int32, device="cuda"), col1[:0], s1[:0])
    E1, E2 = col1.shape[0], col2.shape[0]
    ea = torch.randn((E1 + E2, D), device="cuda")
    conv = _conv(F, H, N, D, 9, False)
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
