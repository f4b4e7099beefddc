"""Host-side checks of wholegraph_amd.nn.TransformerConv (no GPU): PyG's parameter names and shapes over the option grid, the
refusals (beta, attention dropout while training), the aggregate-first folds the layer builds (``nn.transformer_folds``)
against the float64 restatement (tests/transformer_ref.py), and the restatement against a dense attention built by hand."""
import itertools
import math

import pytest
import torch

from transformer_ref import dense_attention, params_of, transformer_forward


@pytest.mark.parametrize("fin,C,H,concat,edge_dim,bias", list(itertools.product(
    [16, (12, 20)], [8], [1, 3], [True, False], [None, 1, 4], [True, False])))
def test_parameters_match_pyg(fin, C, H, concat, edge_dim, bias):
    from wholegraph_amd.nn import TransformerConv
    torch.manual_seed(0)
    conv = TransformerConv(fin, C, heads=H, concat=concat, edge_dim=edge_dim, bias=bias)
    fs, fd = (fin, fin) if isinstance(fin, int) else fin
    HC = H * C
    want = {"lin_key.weight": (HC, fs), "lin_key.bias": (HC,), "lin_query.weight": (HC, fd), "lin_query.bias": (HC,),
            "lin_value.weight": (HC, fs), "lin_value.bias": (HC,), "lin_skip.weight": (HC if concat else C, fd)}
    if bias:
        want["lin_skip.bias"] = (HC if concat else C,)
    if edge_dim is not None:
        want["lin_edge.weight"] = (HC, edge_dim)
    sd = conv.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    # torch.nn.Linear's initialisation: U(-1/sqrt(in), 1/sqrt(in)) for weight and bias
    for k, v in sd.items():
        fan_in = v.shape[1] if v.dim() == 2 else sd[k.replace("bias", "weight")].shape[1]
        assert float(v.abs().max()) <= 1.0 / math.sqrt(fan_in) + 1e-7, k
    new = {k: torch.randn(v) for k, v in want.items()}
    conv.load_state_dict(new)
    for k, v in new.items():
        mod, name = k.split(".")
        assert torch.equal(getattr(getattr(conv, mod), name).detach(), v)


def test_refusals():
    from wholegraph_amd.nn import TransformerConv
    with pytest.raises(NotImplementedError, match="beta"):
        TransformerConv(8, 8, beta=True)
    conv = TransformerConv(8, 8, dropout=0.1)
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(NotImplementedError, match="dropout"):
        conv(torch.randn(2, 8), ei)
    with pytest.raises(TypeError, match="aggr"):
        TransformerConv(8, 8, aggr="mean")
    with pytest.raises(TypeError, match="unsupported"):
        TransformerConv(8, 8, head=2)
    TransformerConv(8, 8, aggr="add", node_dim=0)          # PyG's defaults
    doc = TransformerConv.__doc__
    assert "beta=True" in doc and "dropout" in doc and "library ops" in doc
    conv2 = TransformerConv(8, 8)
    with pytest.raises(ValueError, match="featureless"):
        conv2(None, ei)
    with pytest.raises(ValueError, match="featureless"):
        conv2(torch.arange(2), ei)


def _graph(n_src, n_dst, E, seed, empty=(1, 4, 7)):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n_src, (E,), generator=g)
    dst = torch.randint(0, n_dst, (E,), generator=g)
    for r in empty:                                 # rows with no edges
        dst[dst == r] = (r + 1) % n_dst
    dst[:5] = 0
    src[:2] = 3                                     # a duplicate edge into row 0
    return torch.stack([src, dst])


def _aggregate_first(conv, xs, xd, ei, ea):
    """The layer as the kernel computes it, from ``nn.transformer_folds``: per destination u, w; per edge the logit
    u . x_j + w . a_ij; rows A = [sum alpha [x_j | a_ij | 1 | 0] per head | x_dst]; out = A @ Wstack + bias."""
    from wholegraph_amd.nn import transformer_block_width, transformer_folds
    Fu, bu, Fw, bw, wt, bias = transformer_folds(conv)
    H, Fs, D = conv.heads, xs.shape[1], conv.edge_dim or 0
    W4 = transformer_block_width(Fs, D)
    src, dst = ei[0], ei[1]
    n, E = xd.shape[0], src.shape[0]
    u = (xd @ Fu + bu).view(n, H, Fs)
    s = (u[dst] * xs[src].unsqueeze(1)).sum(-1)
    ext = torch.cat([ea.view(E, D) if D else xs.new_zeros((E, 0)), xs.new_ones((E, 1)), xs.new_zeros((E, W4 - Fs - D - 1))], 1)
    if D:
        w = (xd @ Fw + bw).view(n, H, D)
        s = s + (w[dst] * ea.view(E, 1, D)).sum(-1)
    smax = s.new_full((n, H), -math.inf).scatter_reduce(0, dst.unsqueeze(1).expand(E, H), s, "amax", include_self=True)
    ex = (s - smax[dst]).exp()
    alpha = ex / s.new_zeros((n, H)).index_add(0, dst, ex)[dst]
    rows = torch.cat([xs[src], ext], 1)                                      # [E, W4]
    A = xs.new_zeros((n, H, W4)).index_add(0, dst, alpha.unsqueeze(2) * rows.unsqueeze(1)).reshape(n, H * W4)
    if conv.root_weight:
        A = torch.cat([A, xd], 1)
    out = A @ wt.t()
    return (out if bias is None else out + bias), alpha


@pytest.mark.parametrize("H,concat,D,root,bias,bip", [(3, False, 2, True, True, False), (3, True, None, True, False, True),
                                                      (1, False, 1, True, True, False), (2, True, 4, False, True, True)])
def test_aggregate_first_folds_match_restatement(H, concat, D, root, bias, bip):
    """50 source and 20 destination rows, F = 12, C = 5, three destinations without edges: the folds ``nn`` builds, composed
    aggregate-first, equal PyG's formulation in float64 on the output and on alpha; lin_key's bias gets an exactly zero
    gradient through the folds."""
    from wholegraph_amd.nn import TransformerConv
    torch.manual_seed(H + (D or 0))
    fin = (12, 8) if bip else 12
    conv = TransformerConv(fin, 5, heads=H, concat=concat, edge_dim=D, bias=bias, root_weight=root).double()
    with torch.no_grad():
        for p in conv.parameters():
            p.uniform_(-0.6, 0.6)
    xs = torch.randn(50, 12, dtype=torch.float64)
    xd = torch.randn(20, 8, dtype=torch.float64) if bip else xs[:20]
    ei = _graph(50, 20, 120, seed=H)
    ea = torch.randn(120, D, dtype=torch.float64) if D else None
    got, ga = _aggregate_first(conv, xs, xd, ei, ea)
    ref, ra = transformer_forward(xs, xd, ei, params_of(conv), H, concat, ea, return_alpha=True)
    assert float((got - ref).detach().abs().max()) <= 1e-12 * max(1.0, float(ref.detach().abs().max()))
    assert float((ga - ra).detach().abs().max()) <= 1e-12
    for r in (1, 4, 7):                                  # no edges: the skip term alone (or zero)
        want = conv.lin_skip(xd[r]) if root else torch.zeros_like(got[r])
        assert torch.allclose(got[r], want, atol=1e-12)
    got.sum().backward()
    assert conv.lin_key.bias.grad is not None and bool((conv.lin_key.bias.grad == 0).all())


@pytest.mark.parametrize("H,concat,D", [(1, True, None), (2, False, 3), (3, True, 1)])
def test_restatement_against_dense_attention(H, concat, D):
    """6 nodes: a loop (2 -> 2), duplicates (0 -> 1 twice), node 5 without in-edges, node 4 with one edge."""
    from wholegraph_amd.nn import TransformerConv
    torch.manual_seed(1)
    conv = TransformerConv(4, 3, heads=H, concat=concat, edge_dim=D).double()
    pairs = [(0, 1), (0, 1), (2, 1), (3, 1), (2, 2), (0, 2), (1, 4), (5, 0), (4, 0), (1, 3)]
    ei = torch.tensor([[a for a, _ in pairs], [b for _, b in pairs]])
    x = torch.randn(6, 4, dtype=torch.float64)
    ea = torch.randn(len(pairs), D, dtype=torch.float64) if D else None
    p = params_of(conv)
    got = transformer_forward(x, None, ei, p, H, concat, ea)
    want = dense_attention(x, None, ei, p, H, concat, ea)
    assert torch.allclose(got, want, atol=1e-12)
    assert torch.allclose(got[5], x[5] @ p["Ws"].double().t() + p["bs"].double(), atol=1e-12)   # no in-edges: skip only
    scale = transformer_forward(x, None, ei, p, H, concat, ea, abs_terms=True)
    assert bool((got.abs() <= scale + 1e-12).all())
