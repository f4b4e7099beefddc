"""GPU parity of wholegraph_amd.nn.PNAConv (csrc/wg_pna.hip) against the float64 restatement of PyG's PNAConv (tests/pna_ref.py) at
the bars of test_gpu_transformer.py — ``_close`` (|err| <= 1e-5 x the magnitude sum of the terms + 1e-7), ``_close_grad``
(max |err| <= 1e-4 max |ref|) — over its hop (degrees 0 .. 24, one row of 3000 edges, a hub source, loops and duplicates,
700 rows: a ragged last tile for workgroups of 16, 32 and 64 rows), amended to hold a row of degree 1 (row 0), a row whose edges
are all one source (row 2) and a row without edges (row 3).  Where min, max or their gradients are compared, x and the pre_nns
parameters lie on dyadic grids (multiples of 1/8 and of 1/4 in [-1, 1]): y and a are then exact in float32 whatever the summation
order, ties do occur and both sides resolve them by the lowest slot; nothing is masked out."""
import pytest

from pna_ref import params_of, pna_forward
from test_gpu_transformer import _close, _close_grad, _edge_index, _hop

pytestmark = pytest.mark.gpu

N_DST, N_SRC = 700, 1600
ALL = ["sum", "mean", "min", "max", "var", "std"]
DEF = ["mean", "min", "max", "std"]
S3 = ["identity", "amplification", "attenuation"]
# (F, N, aggregators, scalers, constructor keywords, graph form, relu, lazy, route)
CASES = [(256, 256, ALL, S3, dict(), "layer", False, False, "layer"),                       # M = 1, the LDS maximum
         (64, 48, DEF, S3, dict(), "coo", True, False, "layer"),                            # M = 4, N no multiple of 16; (x_src, x_dst)
         (20, 36, ["max", "std"], ["attenuation"], dict(), "csr", False, False, "layer"),   # F, N no multiples of 16
         (4, 8, ["sum", "min", "var"], ["linear", "inverse_linear"], dict(), "layer", True, True, "layer"),      # one float4 per row
         (16, 32, DEF, S3, dict(towers=4), "layer", False, False, "aggregate"),             # y 64 wide over four towers
         (32, 32, ALL, ["identity", "linear"], dict(post_layers=2), "csr", True, False, "aggregate"),
         (260, 64, DEF, S3, dict(), "coo", False, False, "torch"),                          # outside the domain, the same bars
         (48, 32, ["mean", "std"], S3, dict(), "layer", True, False, "layer")]              # randn inputs (no min / max)


def _pna_hop(n_dst, max_deg, seed, hub=0):
    """``_hop`` with one edge put in front (row 0: degree 1) and row 2's edges all from source 11."""
    import torch
    rp, col, self_rows = _hop(n_dst, N_SRC, max_deg, seed, hub=hub)
    col, rp = torch.cat([col.new_tensor([7]), col]), rp.clone()
    rp[1:] += 1
    col[int(rp[2]):int(rp[3])] = 11
    return rp, col.contiguous(), self_rows


def _grid(shape, step, gen):
    import torch
    return torch.randint(-step, step + 1, shape, generator=gen, device="cuda").float() / step


@pytest.fixture
def launches(monkeypatch):
    """Counts the one-launch forwards (``pna_layer_forward`` calls, their statistics-only outputs kept) and records the backward
    launches of the test (workgroups, a copy of ``gy``); ``launches["max_blocks"]`` forces the backward grid."""
    import wholegraph_amd.nn as wnn
    seen, fwd, bwd = {"fwd": 0, "stats": [], "blocks": [], "gy": [], "max_blocks": None}, wnn.pna_layer_forward, wnn.pna_bwd_src

    def forward(*a, **kw):
        seen["fwd"] += 1
        res = fwd(*a, **kw)
        if kw.get("w_post", a[8] if len(a) > 8 else None) is None:
            seen["stats"].append(res[0] if isinstance(res, tuple) else res)
        return res

    def backward(*a, **kw):
        res = bwd(*a, **dict(kw, max_blocks=seen["max_blocks"]))
        seen["blocks"].append(res[1])
        seen["gy"].append(res[0].clone())
        return res
    monkeypatch.setattr(wnn, "pna_layer_forward", forward)
    monkeypatch.setattr(wnn, "pna_bwd_src", backward)
    return seen


@pytest.mark.parametrize("case", range(len(CASES)))
def test_layer_vs_fp64(hiplib, launches, case):
    """Forward and the gradients of x, pre_nns, post_nns and lin over one hop; one forward launch per hop; two runs with the same
    bits; a third run with the backward on 3 workgroups (100 tiles at a fixed stride): the same bits again."""
    import torch
    from wholegraph_amd import nn
    F, N, aggr, scalers, kw, form, relu, lazy, route = CASES[case]
    rp, col, self_rows = _pna_hop(N_DST, 24, seed=case, hub=3000)
    if form != "layer":                                        # COO and CSR pairs: the destinations are the first rows of x
        self_rows = torch.arange(N_DST, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(case)
    torch.manual_seed(case)
    conv = nn.PNAConv(F, N, aggr, scalers, torch.bincount((rp[1:] - rp[:-1]).long()).cpu(), **kw).cuda()
    x0 = torch.randn((N_SRC, F), device="cuda")
    if set(aggr) & {"min", "max"}:
        x0 = _grid((N_SRC, F), 8, gen)
        with torch.no_grad():
            for p in conv.pre_nns.parameters():
                p.copy_(_grid(p.shape, 4, gen))
    ei = _edge_index(rp, self_rows, col)
    G = torch.randn((N_DST, N), device="cuda")
    graph = {"coo": ei[:, torch.sort(-ei[1], stable=True).indices].contiguous(), "csr": [rp, col],
             "layer": nn.LayerGraph([nn.HopGraph(rp, col, self_rows)])}[form]
    ids = torch.randperm(5000, device="cuda")[:N_SRC]          # lazy: x0 = table[ids], read through ids
    table = torch.zeros((5000, F), device="cuda")
    table[ids] = x0
    runs = []
    for k in range(3):
        launches["max_blocks"] = 3 if k == 2 else None
        conv.zero_grad(set_to_none=True)
        xs = x0.clone().requires_grad_(True)
        xin = nn.LazyRows(table, ids) if lazy else ((xs, xs[:N_DST]) if form == "coo" else xs)
        out = conv(xin, graph, act="relu" if relu else None)
        (out * G).sum().backward()
        runs.append(dict({n: p.grad.clone() for n, p in conv.named_parameters()}, out=out.detach().clone(),
                         **({} if lazy else {"x": xs.grad.clone()})))
    inside = route != "torch"
    assert conv.route == route
    assert launches["fwd"] == (3 if inside else 0) and launches["blocks"] == ([100, 100, 3] if inside else [])
    for n in runs[0] if inside else []:                        # (the kernels'; the torch route adds with index_add)
        assert torch.equal(runs[0][n], runs[1][n]), "not run-to-run deterministic: " + n
        assert torch.equal(runs[0][n], runs[2][n]), "depends on the backward grid: " + n
    if route == "aggregate" and "std" in aggr:                 # phase 1's output: degree 1, one repeated source, no edges
        W = launches["stats"][0].shape[1] // len(aggr)
        std = launches["stats"][0][:, aggr.index("std") * W:][:, :W]
        floor = torch.tensor(1e-5, dtype=torch.float32).sqrt().cuda()
        assert bool((std[0] == floor).all()) and bool((std[2] == floor).all()) and bool((std[3] == 0).all())
    if lazy:                                                   # the statistics read through a node list: the same bits as by row
        y = torch.randn((N_SRC, F), device="cuda")
        big = torch.zeros((5000, F), device="cuda")
        big[ids] = y
        assert torch.equal(nn.pna_layer_forward(rp, col, big, None, aggr, src_ids=ids), nn.pna_layer_forward(rp, col, y, None, aggr))
    p64 = {n: v.double().requires_grad_(True) for n, v in params_of(conv).items()}
    x64 = x0.double().requires_grad_(True)
    where = torch.zeros(N_SRC, dtype=torch.int64, device="cuda")
    where[self_rows] = torch.arange(N_DST, device="cuda")
    am = conv.aggr_module
    ref, scale = pna_forward(x64, x64[self_rows], torch.stack([ei[0], where[ei[1]]]), p64, aggr, scalers, float(am.avg_deg_lin),
                             float(am.avg_deg_log), towers=kw.get("towers", 1), relu=relu)
    (ref * G.double()).sum().backward()
    assert sorted(runs[0]) == sorted(list(p64) + ["out"] + ([] if lazy else ["x"]))
    for got in (runs[0], runs[2]):
        _close(got["out"], ref.detach(), scale, "forward")
        for n, v in p64.items():
            _close_grad(got[n], v.grad, "d" + n)
        if not lazy:
            _close_grad(got["x"], x64.grad, "dx")


def test_two_hop_layer_graph(hiplib, launches):
    """A two-hop LayerGraph (an empty hop between, self_rows no identity): each hop's output rows and each hop's backward launch
    (its share of dy, before the library GEMMs that turn the hops' sum into dx) equal the layer run on that hop alone bit for
    bit, dx their sum at the gradient bar; an empty hop makes no launch."""
    import torch
    from wholegraph_amd import nn
    rp1, col1, s1 = _pna_hop(N_DST, 24, seed=7, hub=3000)
    rp2, col2, s2 = _hop(300, N_SRC, 9, seed=8)
    h1, h2 = nn.HopGraph(rp1, col1, s1), nn.HopGraph(rp2, col2, s2)
    none = nn.HopGraph(torch.zeros(1, dtype=torch.int32, device="cuda"), col1[:0], s1[:0])
    torch.manual_seed(9)
    gen = torch.Generator(device="cuda").manual_seed(9)
    conv = nn.PNAConv(16, 16, ALL, S3, torch.bincount((rp1[1:] - rp1[:-1]).long()).cpu()).cuda()
    with torch.no_grad():
        for p in conv.pre_nns.parameters():
            p.copy_(_grid(p.shape, 4, gen))
    x = _grid((N_SRC, 16), 8, gen)
    G = torch.randn((N_DST + 300, 16), device="cuda")

    def run(hops, g):
        conv.zero_grad(set_to_none=True)
        xs = x.clone().requires_grad_(True)
        out = conv(xs, nn.LayerGraph(hops), act="relu")
        (out * g).sum().backward()
        return out.detach(), xs.grad
    both, first, second = run([h1, none, h2], G), run([h1], G[:N_DST]), run([h2], G[N_DST:])
    assert launches["fwd"] == 4 and len(launches["gy"]) == 4
    assert torch.equal(both[0][:N_DST], first[0]) and torch.equal(both[0][N_DST:], second[0])
    assert torch.equal(launches["gy"][0], launches["gy"][2]) and torch.equal(launches["gy"][1], launches["gy"][3])
    _close_grad(both[1], first[1].double() + second[1].double(), "dx of both hops")
