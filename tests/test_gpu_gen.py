"""GPU parity of wholegraph_amd.nn.GENConv (csrc/wg_gen.hip) against the float64 restatement of PyG's GENConv with the softmax
aggregator (tests/gen_ref.py) at the bars of test_gpu_transformer.py — ``_close`` (|err| <= 1e-5 x the magnitude sum of the terms +
1e-7), ``_close_grad`` (max |err| <= 1e-4 max |ref|) — over its hop: rows of degree 0 and 24 (across the eight-edge unroll), one row
of 3000 edges, a hub source (the 64-entry pieces of the backward), sampled loops and duplicates, 700 = 43 x 16 + 12 rows.  The
graph's form, the trailing ReLU, the temperature and a LazyRows input rotate through the cases."""
import pytest

from gen_ref import gen_forward, params_of
from test_gpu_transformer import _close, _close_grad, _edge_index, _hop

pytestmark = pytest.mark.gpu

N_DST, N_SRC = 700, 1600
# (in_channels, C, constructor keywords, t, learn_t, graph form, relu, lazy, route)
CASES = [(256, 256, dict(expansion=1), 1.0, False, "layer", False, False, "mlp"),        # all lanes busy, the LDS maximum
         (20, 20, dict(expansion=1.8, bias=True), 0.25, True, "csr", True, False, "mlp"),  # C, H = 36 no multiples of 16
         (4, 4, dict(), -1.0, True, "layer", False, True, "mlp"),                          # one float4 per row, rows read through ids
         (48, 32, dict(bias=True), 4.0, False, "layer", True, True, "mlp"),                # lin_src / lin_dst over the lazy table
         (16, 16, dict(norm="batch"), 0.0, True, "coo", False, False, "aggregate"),        # the mlp outside; t = 0: the mean
         (260, 260, dict(expansion=1), 1.0, True, "coo", True, False, "torch"),            # outside the domain, the same bars
         (32, 32, dict(), 100.0, True, "layer", False, False, "mlp")]                      # overflow: x from {-1, 0, 1}, exact ties


@pytest.fixture
def launches(monkeypatch):
    """Counts the one-launch forwards (``gen_layer_forward`` calls) and the workgroups of the backward launches of the test;
    ``launches["max_blocks"]`` forces the backward grid."""
    import wholegraph_amd.nn as wnn
    seen, fwd, bwd = {"fwd": 0, "blocks": [], "max_blocks": None}, wnn.gen_layer_forward, wnn.gen_bwd_src

    def forward(*a, **kw):
        seen["fwd"] += 1
        return fwd(*a, **kw)

    def backward(*a, **kw):
        res = bwd(*a, **dict(kw, max_blocks=seen["max_blocks"]))
        seen["blocks"].append(res[1].shape[0])
        return res
    monkeypatch.setattr(wnn, "gen_layer_forward", forward)
    monkeypatch.setattr(wnn, "gen_bwd_src", backward)
    return seen


@pytest.mark.parametrize("case", range(len(CASES)))
def test_layer_vs_fp64(hiplib, launches, case):
    """Forward and the gradients of x, mlp, lin_src, lin_dst and t over one hop; one forward launch per hop; two runs with the same
    bits; a third run with the backward on 3 workgroups (100 tiles at a fixed stride): the same dx bits, dt inside the bar."""
    import torch
    from wholegraph_amd import nn
    cin, C, kw, t, learn_t, form, relu, lazy, route = CASES[case]
    rp, col, self_rows = _hop(N_DST, N_SRC, 24, seed=case, hub=3000)
    if form != "layer":                                        # COO and CSR pairs: the destinations are the first rows of x
        self_rows = torch.arange(N_DST, device="cuda")
    torch.manual_seed(case)
    conv = nn.GENConv(cin, C, t=t, learn_t=learn_t, **kw).cuda()
    x0 = torch.randn((N_SRC, cin), device="cuda") if t < 100 else torch.randint(-1, 2, (N_SRC, cin), device="cuda").float()
    ei = _edge_index(rp, self_rows, col)
    G = torch.randn((N_DST, C), device="cuda")
    graph = {"coo": ei[:, torch.sort(-ei[1], stable=True).indices].contiguous(), "csr": [rp, col],
             "layer": nn.LayerGraph([nn.HopGraph(rp, col, self_rows)])}[form]
    ids = torch.randperm(5000, device="cuda")[:N_SRC]          # lazy: x0 = table[ids], read through ids
    table = torch.zeros((5000, cin), device="cuda")
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
        assert n == "aggr_module.t" or torch.equal(runs[0][n], runs[2][n]), "depends on the backward grid: " + n
    p64 = {n: v.double().requires_grad_(True) for n, v in params_of(conv).items()}
    x64, t64 = x0.double().requires_grad_(True), conv.t.detach().double().requires_grad_(True)
    where = torch.zeros(N_SRC, dtype=torch.int64, device="cuda")
    where[self_rows] = torch.arange(N_DST, device="cuda")
    ref, scale = gen_forward(x64, x64[self_rows], torch.stack([ei[0], where[ei[1]]]), p64, t64, relu=relu)
    (ref * G.double()).sum().backward()
    assert sorted(runs[0]) == sorted(list(p64) + ["out"] + (["aggr_module.t"] if learn_t else []) + ([] if lazy else ["x"]))
    for got in (runs[0], runs[2]):
        _close(got["out"], ref.detach(), scale, "forward")
        for n, v in p64.items():
            _close_grad(got[n], v.grad, "d" + n)
        if learn_t:
            _close_grad(got["aggr_module.t"], t64.grad.reshape(1), "dt")
        if not lazy:
            _close_grad(got["x"], x64.grad, "dx")


def test_two_hop_layer_graph(hiplib, launches):
    """A two-hop LayerGraph (an empty hop between, self_rows no identity): each hop's rows and its share of every gradient equal
    the layer run on that hop alone; an empty hop makes no launch."""
    import torch
    from wholegraph_amd import nn
    rp1, col1, s1 = _hop(N_DST, N_SRC, 24, seed=7, hub=3000)
    rp2, col2, s2 = _hop(300, N_SRC, 9, seed=8)
    h1, h2 = nn.HopGraph(rp1, col1, s1), nn.HopGraph(rp2, col2, s2)
    none = nn.HopGraph(torch.zeros(1, dtype=torch.int32, device="cuda"), col1[:0], s1[:0])
    torch.manual_seed(9)
    conv = nn.GENConv(16, 16, t=0.5, learn_t=True).cuda()
    x = torch.randn((N_SRC, 16), device="cuda")
    G = torch.randn((N_DST + 300, 16), device="cuda")

    def run(hops, g):
        conv.zero_grad(set_to_none=True)
        xs = x.clone().requires_grad_(True)
        out = conv(xs, nn.LayerGraph(hops), act="relu")
        (out * g).sum().backward()
        return out.detach(), xs.grad, conv.t.grad.clone()
    both, first, second = run([h1, none, h2], G), run([h1], G[:N_DST]), run([h2], G[N_DST:])
    assert launches["fwd"] == 4
    assert torch.equal(both[0][:N_DST], first[0]) and torch.equal(both[0][N_DST:], second[0])
    assert torch.equal(both[1], first[1] + second[1])
    a, b = float(first[2]), float(second[2])                   # dt: the hops' sums added once in float32
    assert abs(float(both[2]) - (a + b)) <= 2.0 ** -23 * (abs(a) + abs(b))
