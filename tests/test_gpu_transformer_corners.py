"""The corners of the transformer kernels' domain (``tconv_row_walk``, ``tconv_bwd_dst_kernel``, ``hetero_tconv_kernel``: D <= 32,
F <= 256, H <= 8, K <= 1024, N <= 256), which the other transformer tests stay away from.

Homogeneous layer, through ``nn.TransformerConv`` with the helpers of tests/test_gpu_transformer.py: forward and alpha at the bars of
``test_layer_forward_vs_fp64`` (|err| <= 1e-5 x the magnitude sum of the terms + 1e-7; alpha within 1e-5), the full backward at the
bars of ``test_layer_backward_vs_fp64_and_deterministic`` (max |err| <= 1e-4 x max |reference gradient|, bitwise repeat), on the
one-kernel route.  Hetero launch, through ``nn.hetero_transformer_launch`` against tests/hetero_launch_ref.py: ``out`` within 1e-5 x
the magnitude sum of its terms, alpha within 1e-5, the kept A within 1e-5 x its magnitude sum, exact zeros where a relation has
no edge, the ``_train`` form's bits equal to the inference form's."""
import pytest

from hetero_launch_ref import block_width, edge_case_hop, hetero_transformer_launch_ref
from test_gpu_transformer import _close, _close_grad, _conv, _count_launches, _edge_index
from transformer_ref import params_of, transformer_forward

pytestmark = pytest.mark.gpu

# rows of degree 0, 1, 3, 4, 5, 8, 9 (the groups of 4 edges and their remainders), one row of 3000 edges (the online softmax over
# 750 groups), 21 rows: a full tile and five rows of a second one
DEGREES = [0, 1, 3, 4, 5, 8, 9, 3000, 0, 2, 16, 17, 7, 4, 1, 0, 12, 5, 0, 3, 6]
N_DST, N_SRC = len(DEGREES), 64

# (heads, concat, edge_dim, F_src, C, bipartite F_dst or None)
CORNERS = [
    (8, True, 32, 64, 32, None),        # D at its limit, H at its limit, N = 256, K = 8 x 100 + 64 = 864
    (2, False, 31, 256, 64, None),      # every lane carries x, 32 lanes carry [a | 1]; K = 2 x 288 + 256 = 832
    (3, False, 3, 252, 40, 256),        # bipartite, K = 3 x 256 + 256 = 1024 exactly
    (7, True, None, 16, 8, None),       # head counts inside bucket 8
    (6, False, 5, 32, 24, None),
    (1, False, 32, 4, 1, None),         # the smallest F with the largest D, N = 1
    (1, True, 2, 16, 12, None),         # K = 20 + 16 = 36: K % 16 == 4
]


def corner_k(H, D, F, Fd):
    return H * block_width(F, D or 0) + (F if Fd is None else Fd)


@pytest.mark.parametrize("case", range(len(CORNERS)))
def test_layer_corner_forward_backward_vs_fp64(hiplib, case, monkeypatch):
    import torch
    from wholegraph_amd import nn
    H, concat, D, F, C, Fd = CORNERS[case]
    N = H * C if concat else C
    K = corner_k(H, D, F, Fd)
    assert nn.transformer_layer_supported(F, F if Fd is None else Fd, D or 0, H, N) and K <= 1024
    assert K == [864, 832, 1024, 156, 272, 44, 36][case]
    g = torch.Generator().manual_seed(50 + case)
    rp, col = (t.cuda() for t in edge_case_hop(N_DST, N_SRC, DEGREES, seed=case))
    E = int(col.shape[0])
    self_rows = (torch.arange(N_DST) if Fd is not None else torch.randperm(N_SRC, generator=g)[:N_DST]).cuda()
    ei = _edge_index(rp, self_rows, col)
    conv = _conv(F if Fd is None else (F, Fd), C, H, concat, D, seed=60 + case)
    x0 = torch.randn((N_SRC, F), generator=g).cuda()
    xd0 = torch.randn((N_DST, Fd), generator=g).cuda() if Fd else None
    ea0 = torch.randn((E, D), generator=g).cuda() if D else None
    G = torch.randn((N_DST, N), generator=g).cuda()
    lg = nn.LayerGraph([nn.HopGraph(rp, col, self_rows)])
    launches = _count_launches(monkeypatch)
    p = params_of(conv)

    # forward and alpha (the bars of test_layer_forward_vs_fp64)
    with torch.no_grad():
        if Fd is not None:
            got, (_, alpha) = conv((x0, xd0), ei, ea0, return_attention_weights=True)
        else:
            got, alpha = conv(x0, lg, ea0, return_attention_weights=True)
    ref, ra = transformer_forward(x0, xd0, ei, p, H, concat, ea0, return_alpha=True)
    scale = transformer_forward(x0, xd0, ei, p, H, concat, ea0, abs_terms=True)
    if Fd is None:
        ref, scale = ref[self_rows], scale[self_rows]
    assert got.shape == (N_DST, N) and len(launches) == 1, "the one-kernel route"
    err = (got.double() - ref).abs()
    print("corner %d (H %d D %s F %d K %d N %d): forward max |err| %.3e, worst err / magnitude sum %.3e, alpha max |err| %.3e"
          % (case, H, D, F, K, N, float(err.max()), float((err / scale.clamp(min=1e-30)).max()), float((alpha.double() - ra).abs().max())))
    _close(got, ref, scale, "forward")
    assert float((alpha.double() - ra).abs().max()) <= 1e-5, "alpha"

    # the full backward (the bars of test_layer_backward_vs_fp64_and_deterministic), twice
    runs = []
    for _ in range(2):
        conv.zero_grad(set_to_none=True)
        ea = None if ea0 is None else ea0.clone().requires_grad_(True)
        xs = x0.clone().requires_grad_(True)
        if Fd is not None:
            xd = xd0.clone().requires_grad_(True)
            out, xg = conv((xs, xd), ei, ea), [xs, xd]
        else:
            out, xg = conv(xs, lg, ea), [xs]
        (out * G).sum().backward()
        grads = {k: q.grad.clone() for k, q in conv.named_parameters()}
        for k, t in enumerate(xg):
            grads["x%d" % k] = t.grad.clone()
        if ea is not None:
            grads["edge_attr"] = ea.grad.clone()
        runs.append((out.detach().clone(), grads))
    assert len(launches) == 3, "the one-kernel route"
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), "backward is not run-to-run deterministic: " + k
    p64 = {k: None if v is None else v.double().requires_grad_(True) for k, v in p.items()}
    x64 = x0.double().requires_grad_(True)
    xd64 = None if xd0 is None else xd0.double().requires_grad_(True)
    ea64 = None if ea0 is None else ea0.double().requires_grad_(True)
    ref = transformer_forward(x64, xd64, ei, p64, H, concat, ea64)
    if Fd is None:
        ref = ref[self_rows]
    (ref * G.double()).sum().backward()
    names = {"lin_query.weight": "Wq", "lin_query.bias": "bq", "lin_key.weight": "Wk", "lin_value.weight": "Wv",
             "lin_value.bias": "bv", "lin_edge.weight": "We", "lin_skip.weight": "Ws", "lin_skip.bias": "bs"}
    got_g = runs[0][1]
    wanted = [(k, p64[r].grad) for k, r in names.items() if k in got_g] + [("x0", x64.grad)]
    if Fd is not None:
        wanted.append(("x1", xd64.grad))
    if D:
        wanted.append(("edge_attr", ea64.grad))
    for k, want in wanted:
        print("corner %d d%s: max |err| %.3e, largest reference gradient %.3e"
              % (case, k, float((got_g[k].double() - want).abs().max()), float(want.abs().max())))
    for k, want in wanted:
        _close_grad(got_g[k], want, "d" + k)
    assert float(got_g["lin_key.bias"].abs().max()) <= 1e-4 * float(got_g["lin_key.weight"].abs().max()), "dlin_key.bias"


# ---- the hetero launch ---------------------------------------------------------------------------------------------------------
N_ROWS = 37
CYCLE = [0, 1, 3, 4, 5, 9, 17]         # hand_built's degrees (tests/test_gpu_hetero_transformer.py), offset per relation

# (name, [(H, F, D) per relation], F_dst, N)
LAUNCHES = [
    # eight relations; the H = 1 ones run under the HM = 8 instantiation relation 0 asks for; D rotates through 0, 1, 32
    ("eight-relations", [(8, 8, 0), (1, 8, 1), (3, 8, 32), (1, 8, 0), (2, 8, 1), (1, 8, 32), (5, 8, 0), (1, 8, 1)], 8, 47),
    # two relations of F = 256, H = 1, D = 32 and a 256-wide root: K = 2 x 292 + 256 = 840
    ("wide", [(1, 256, 32), (1, 256, 32)], 256, 256),
    # K = 256 + 512 + 128 + 128 = 1024 exactly
    ("K1024", [(4, 60, 3), (2, 252, 3), (1, 124, 0)], 128, 32),
]


def build_launch(spec, dev):
    import torch
    name, rel_specs, F_dst, N = spec
    g = torch.Generator().manual_seed(len(name))
    rels, at = [], 0
    for r, (H, F, D) in enumerate(rel_specs):
        n_src = 30 + 5 * r
        deg = [CYCLE[(i + 2 * r) % 7] for i in range(N_ROWS)]
        for i in (20, 36):                       # rows without an edge in any relation
            deg[i] = 0
        deg[(5 + 3 * r) % N_ROWS] = 3000 if r == 0 else 0      # one 3000-edge row; the others have no edge there ...
        if r == 1:
            deg[5] = 0                                          # ... and relation 1 none in relation 0's heavy row
        row_ptr, col = edge_case_hop(N_ROWS, n_src, deg, seed=10 * r + len(name))
        E = int(col.shape[0])
        x = torch.randn((n_src, F), generator=g)
        ids = None
        kind = [None, torch.int32, torch.int64][r % 3]
        if kind is not None:
            ids = torch.randperm(2 * n_src, generator=g)[:n_src].to(kind)
            table = torch.full((2 * n_src, F), float("nan"))
            table[ids.long()] = x
            x = table
        ea = torch.randn((E, D), generator=g) if D else None
        # u: a column slice of a wider product (ldu > H F, rows 16-B aligned); logits of order 1
        u = (torch.randn((N_ROWS, H * F + 8), generator=g) * (1.5 / F ** 0.5))[:, 4:4 + H * F]
        w = torch.randn((N_ROWS, H * D), generator=g) * 0.5 if D else None
        rels.append([None if t is None else t.to(dev) for t in (row_ptr, col, x, ids, ea, u, w)] + [H, None])
        at += H * block_width(F, D)
    n_dst = N_ROWS + 8
    root = (torch.randn((n_dst, F_dst), generator=g).to(dev), torch.randperm(n_dst, generator=g)[:N_ROWS].contiguous().to(dev), None)
    K = at + F_dst
    wt = (torch.randn((N, K), generator=g) * 0.2).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    out_rows = torch.randperm(N_ROWS + 13, generator=g)[:N_ROWS].contiguous().to(dev)
    return rels, root, wt, bias, out_rows, K


_RESULTS = {}


def launched(spec):
    """The launch of ``spec`` in its inference form and twice in its ``_train`` form, and its float64 restatement, once per session."""
    import torch
    from wholegraph_amd import nn
    name, rel_specs, F_dst, N = spec
    if name in _RESULTS:
        return _RESULTS[name]
    dev = torch.device("cuda", 0)
    rels, root, wt, bias, out_rows, K = build_launch(spec, dev)
    assert K == {"eight-relations": 400, "wide": 840, "K1024": 1024}[name]
    n_out = N_ROWS + 13
    runs = []
    for train in (False, True, True):
        out = torch.full((n_out, N), -123.0, device=dev)
        A = torch.full((N_ROWS, K), -123.0, device=dev) if train else None
        alphas = [torch.full((int(r[1].shape[0]), r[7]), 7.0, device=dev) if train else None for r in rels]
        before = nn.hetero_transformer_launches
        nn.hetero_transformer_launch([tuple(r[:8]) + (al,) for r, al in zip(rels, alphas)], N_ROWS, wt, N, root=root, bias=bias,
                                     relu=True, out_rows=out_rows, out=out, a_save=A)
        assert nn.hetero_transformer_launches - before == 1
        runs.append((out, A, alphas))
    (out, _, _), (out_t, A, alphas), (out_2, A_2, alphas_2) = runs
    assert torch.equal(out, out_t), "the _train form's out differs from the inference form's"
    assert torch.equal(out_t, out_2) and torch.equal(A, A_2) and all(torch.equal(a, b) for a, b in zip(alphas, alphas_2))
    tuples = [tuple(r) for r in rels]
    ref, A64, mag, ralphas = hetero_transformer_launch_ref(tuples, N_ROWS, wt, N, root=root, bias=bias, relu=True, out_rows=out_rows,
                                                           n_out=n_out)
    _, A_abs, _, _ = hetero_transformer_launch_ref(tuples, N_ROWS, wt, N, root=root, bias=bias, out_rows=out_rows, n_out=n_out,
                                                   abs_terms=True)
    _RESULTS[name] = dict(rels=rels, root=root, out_rows=out_rows, K=K, n_out=n_out, out=out, A=A, alphas=alphas, ref=ref, A64=A64,
                          mag=mag, ralphas=ralphas, A_abs=A_abs)
    return _RESULTS[name]


@pytest.mark.parametrize("spec", LAUNCHES, ids=[s[0] for s in LAUNCHES])
def test_hetero_launch_corner_vs_fp64(hiplib, spec):
    """``out`` at 1e-5 x the magnitude sum, alpha within 1e-5, sentinel rows, exact zeros where a relation has no edge, the root
    block a copy; the ``_train`` form's bits equal to the inference form's and to a second run's (``launched``)."""
    import torch
    name, rel_specs, F_dst, N = spec
    b = launched(spec)
    out, A, K = b["out"], b["A"], b["K"]
    named = torch.zeros(b["n_out"], dtype=torch.bool, device=out.device)
    named[b["out_rows"]] = True
    assert bool((out[~named] == -123.0).all()) and int((~named).sum()) == 13
    err = (out[named].double() - b["ref"][named]).abs()
    mag = b["mag"][named]
    worst = float((err / mag.clamp(min=1e-30)).max())
    worst_alpha = max(float((a.double() - r).abs().max()) for a, r in zip(b["alphas"], b["ralphas"]) if a.numel())
    print("%s (K %d): out max |err| %.3e, worst err / magnitude sum %.3e; alpha max |err| %.3e" % (name, K, float(err.max()), worst, worst_alpha))
    assert bool(torch.isfinite(out[named]).all()) and bool((err <= 1e-5 * mag).all()), (name, "out", worst)
    assert worst_alpha <= 1e-5, (name, "alpha", worst_alpha)
    at = 0
    for r, (H, F, D) in zip(b["rels"], rel_specs):
        width = H * block_width(F, D)
        deg = (r[0][1:] - r[0][:-1]).long()
        blk = A[:, at:at + width]
        assert int((deg == 0).sum()) >= 2 and float(blk[deg == 0].abs().max()) == 0.0, (name, "a relation's blocks where it has no edge")
        at += width
    assert torch.equal(A[:, at:], b["root"][0][b["root"][1]])


@pytest.mark.parametrize("spec", LAUNCHES, ids=[s[0] for s in LAUNCHES])
def test_hetero_launch_corner_kept_rows_vs_fp64(hiplib, spec):
    """The kept A within 1e-5 x its magnitude sum (sum_e alpha [|x| | |a| | 1]) of float64, element by element — the 3000-edge
    row whose edges draw from 30 source rows included (1.2e-5 when every term joins the running sums on its own; the walk adds
    a group's four terms first)."""
    name = spec[0]
    b = launched(spec)
    err_a = (b["A"].double() - b["A64"]).abs()
    worst_a = float((err_a / b["A_abs"].clamp(min=1e-30)).max())
    print("%s (K %d): A worst err / magnitude sum %.3e" % (name, b["K"], worst_a))
    assert bool((err_a <= 1e-5 * b["A_abs"]).all()), (name, "A", worst_a)
