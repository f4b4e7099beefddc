"""nn.HeteroConv over TransformerConv relations, the parts that need no GPU: the float64 restatement of
tests/hetero_transformer_ref.py against an edge-by-edge dense attention, the stacking algebra of the one-kernel route
(``nn.hetero_transformer_stack``: rows A times ONE stacked weight = the sum over the relations), the layer on CPU tensors (the
library-ops route), the launch plan, and what the layer refuses about ``edge_attr_dict``."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hetero_transformer_ref as ref  # noqa: E402
import transformer_ref as tref  # noqa: E402

ETS = [("a", "r1", "a"), ("b", "r2", "a"), ("b", "r3", "a")]


def hand_built(g, perm_rows=True):
    """Two source types (a: 13 input rows, b: 9), three relations into type ``a`` over ONE hop of 10 frontier entries; degrees
    0..6, different per relation (row 0 has an edge in r3 alone, row 1 in r1 alone, row 8 in r2 alone), output rows a
    permutation."""
    from wholegraph_amd import nn
    n_in = {"a": 13, "b": 9}
    n = 10
    dst = torch.randperm(n_in["a"], generator=g)[:n]
    rows = torch.randperm(n, generator=g) if perm_rows else None
    degs = {ETS[0]: [0, 1, 3, 4, 5, 0, 2, 1, 0, 2], ETS[1]: [0, 0, 2, 1, 0, 6, 1, 0, 3, 1], ETS[2]: [1, 0, 0, 2, 4, 1, 0, 3, 0, 0]}
    rels, base = [], {}
    for et in ETS:
        rp = torch.zeros(n + 1, dtype=torch.int32)
        rp[1:] = torch.cumsum(torch.tensor(degs[et]), 0)
        col = torch.randint(0, n_in[et[0]], (int(rp[-1]),), generator=g, dtype=torch.int32)
        rels.append(nn.RelationHop(et, 0, rp, col, dst, rows, int(rp[-1]), 6, edge_base=base.get(et, 0)))
    return nn.HeteroLayerGraph(rels, {"a": n, "b": 0}, ["a", "b"]), n_in


def make_layer(widths, heads, C, concat, roots, edge_dims):
    from wholegraph_amd import nn
    convs = {}
    for k, et in enumerate(ETS):
        H = heads[k]
        convs[et] = nn.TransformerConv((widths[et[0]], widths["a"]), C[k], heads=H, concat=concat, root_weight=roots[k],
                                       edge_dim=edge_dims[k])
    return nn.HeteroConv(convs)


def edge_attrs(graph, layer, g):
    return {r.edge_type: torch.randn((r.n_edges, layer.conv(r.edge_type).edge_dim), generator=g)
            for r in graph.relations if layer.conv(r.edge_type).edge_dim is not None}


def test_restatement_matches_dense_attention_summed_over_relations():
    g = torch.Generator().manual_seed(11)
    graph, n_in = hand_built(g)
    widths = {"a": 8, "b": 12}
    torch.manual_seed(2)
    layer = make_layer(widths, [2, 2, 1], [4, 4, 8], True, [True, False, True], [3, None, 1])
    xs = {t: torch.randn((n_in[t], widths[t]), generator=g) for t in n_in}
    ea = edge_attrs(graph, layer, g)
    got = ref.hetero_transformer_forward(xs, graph, ref.params_of(layer), ea)["a"]
    want = torch.zeros((10, 8), dtype=torch.float64)
    r0 = graph.relations[0]
    for r in graph.relations:
        c = layer.conv(r.edge_type)
        coo = ref.relation_coo(r)
        want += tref.dense_attention(xs[r.edge_type[0]], xs["a"][r0.dst_rows], coo, tref.params_of(c), c.heads, concat=True,
                                     edge_attr=ea.get(r.edge_type))
    placed = torch.zeros_like(want).index_copy(0, r0.out_rows, want)
    assert float((got - placed).abs().max()) <= 1e-12 * float(placed.abs().max())
    # a relation's rows without edges get no message and no value bias: row 0 has edges in r3 alone
    only = tref.dense_attention(xs["b"], xs["a"][r0.dst_rows], ref.relation_coo(graph.relations[2]), tref.params_of(layer.conv(ETS[2])),
                                1, edge_attr=ea[ETS[2]])[0]
    skip1 = xs["a"][r0.dst_rows[0]].double() @ layer.conv(ETS[0]).lin_skip.weight.double().t() + layer.conv(ETS[0]).lin_skip.bias.double()
    assert float((got[r0.out_rows[0]] - (only + skip1.detach())).abs().max()) <= 1e-12


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("roots", [(True, True, True), (True, False, True), (False, False, False)])
@pytest.mark.parametrize("edge_dim", [None, 3])
def test_stacked_rows_times_stacked_weight_is_the_sum_over_relations(concat, roots, edge_dim):
    """A = [sum_e alpha [x_j | a_e | 1 | 0] per head, per relation | x_dst] built from the restatement's alphas, wt and bias from
    the layer's own stacking helper, all in float64: A @ wt^T + bias is the restatement's output."""
    from wholegraph_amd import nn
    g = torch.Generator().manual_seed(7)
    graph, n_in = hand_built(g, perm_rows=False)
    widths = {"a": 8, "b": 12}
    torch.manual_seed(4)
    C = [4, 4, 8] if concat else [6, 6, 6]
    layer = make_layer(widths, [2, 2, 1], C, concat, list(roots), [edge_dim, None, edge_dim]).double()
    xs = {t: torch.randn((n_in[t], widths[t]), generator=g, dtype=torch.float64) for t in n_in}
    ea = {et: v.double() for et, v in edge_attrs(graph, layer, g).items()}
    want = ref.hetero_transformer_forward(xs, graph, ref.params_of(layer), ea)["a"]
    convs = [layer.conv(et) for et in ETS]
    with torch.no_grad():
        wt, bias, fold, fold_b, layout = nn.hetero_transformer_stack(convs)
    xd = xs["a"][graph.relations[0].dst_rows]
    K_rel = layout[-1]["col0"] + layout[-1]["width"]
    assert wt.shape == (8 if concat else 6, K_rel + (8 if any(roots) else 0)) and fold.shape[1] % 4 == 0
    A = torch.zeros((10, wt.shape[1]), dtype=torch.float64)
    uw = xd @ fold + fold_b
    for r, c, lay in zip(graph.relations, convs, layout):
        coo = ref.relation_coo(r)
        a_r = ea.get(r.edge_type)
        _, alpha = tref.transformer_forward(xs[r.edge_type[0]], xd, coo, tref.params_of(c), c.heads, concat=concat, edge_attr=a_r,
                                            return_alpha=True)
        F_, D, W4 = lay["F"], lay["D"], lay["W4"]
        assert W4 == (F_ + D + 1 + 3) // 4 * 4 and lay["col0"] % 4 == 0 and lay["u0"] % 4 == 0
        row = torch.cat([xs[r.edge_type[0]][coo[0]]] + ([a_r] if D else []) + [torch.ones((r.n_edges, 1), dtype=torch.float64)], 1)
        # the folds give the restatement's logits: s = u . x_j + w . a_e (+ a per-row constant, lin_key's bias, which cancels)
        u = uw[:, lay["u0"]:lay["u0"] + c.heads * F_].view(10, c.heads, F_)
        s = (u[coo[1]] * xs[r.edge_type[0]][coo[0]].unsqueeze(1)).sum(-1)
        if D:
            s = s + (uw[:, lay["w0"]:lay["w0"] + c.heads * D].view(10, c.heads, D)[coo[1]] * a_r.unsqueeze(1)).sum(-1)
        for i in range(10):
            es = (coo[1] == i).nonzero().view(-1)
            if len(es):
                assert float((torch.softmax(s[es], 0) - alpha[es]).abs().max()) <= 1e-12
        for h in range(c.heads):
            blk = torch.zeros((10, F_ + D + 1), dtype=torch.float64).index_add(0, coo[1], alpha[:, h:h + 1] * row)
            A[:, lay["col0"] + h * W4:lay["col0"] + h * W4 + F_ + D + 1] = blk
    if any(roots):
        A[:, K_rel:] = xd
    got = A @ wt.t() + (0 if bias is None else bias)
    assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0)


def test_cpu_layer_takes_library_ops_and_matches_float64():
    """The fallback on CPU tensors: a relation with F_src = 30 (outside the kernel's domain anyway), out_rows a permutation,
    every element within 1e-5 x the magnitude sum of its terms; no kernel launch."""
    from wholegraph_amd import nn
    g = torch.Generator().manual_seed(3)
    graph, n_in = hand_built(g)
    widths = {"a": 8, "b": 30}
    torch.manual_seed(6)
    for concat, relu in ((True, False), (False, True)):
        layer = make_layer(widths, [2, 2, 1], [4, 4, 8] if concat else [8, 8, 8], concat, [True, False, True], [3, None, 1])
        xs = {t: torch.randn((n_in[t], widths[t]), generator=g) for t in n_in}
        ea = edge_attrs(graph, layer, g)
        before = nn.hetero_transformer_launches
        out = layer(xs, graph, act="relu" if relu else None, edge_attr_dict=ea)
        assert nn.hetero_transformer_launches == before
        assert set(out) == {"a"} and out["a"].shape == (10, 8)
        p = ref.params_of(layer)
        want = ref.hetero_transformer_forward(xs, graph, p, ea, relu=relu)["a"]
        mag = ref.hetero_transformer_forward(xs, graph, p, ea, abs_terms=True)["a"]
        err = (out["a"].detach().double() - want).abs()
        assert bool((err <= 1e-5 * mag).all()), float((err / mag).max())
        out["a"].sum().backward()          # ordinary autograd over the library ops
        assert all(q.grad is not None for q in layer.conv(ETS[0]).lin_value.parameters())


def test_transformer_conv_alone_points_to_hetero_conv():
    from wholegraph_amd import nn
    g = torch.Generator().manual_seed(1)
    graph, n_in = hand_built(g)
    with pytest.raises(NotImplementedError, match="HeteroConv"):
        nn.TransformerConv(8, 4)(torch.randn((13, 8), generator=g), graph)


@pytest.mark.parametrize("F_in,H,D,n_rel,want", [
    (128, 1, 0, 4, 1),      # 4 x 132 + 128 = 656 floats
    (256, 1, 0, 4, 2),      # mag's paper at a hidden width of 256: 4 x 260 + 256 = 1296
    (256, 2, 2, 3, 3),      # 3 x 520 + 256: no two relations fit one launch
])
def test_launch_plan_of_the_stacked_row(F_in, H, D, n_rel, want):
    from wholegraph_amd import nn
    convs = [nn.TransformerConv(F_in, 16, heads=H, concat=False, edge_dim=D or None) for _ in range(n_rel)]
    with torch.no_grad():
        wt, _, _, _, layout = nn.hetero_transformer_stack(convs)
    widths = [lay["width"] for lay in layout]
    assert widths == [H * nn.transformer_block_width(F_in, D)] * n_rel and wt.shape[1] == sum(widths) + F_in
    plan = nn.hetero_sage_plan(widths, F_in, max_k=nn.HETERO_TRANSFORMER_MAX_K)
    assert len(plan) == want
    at = 0
    for k, (lo, hi, root) in enumerate(plan):
        assert lo == at and sum(widths[lo:hi]) + (F_in if root else 0) <= 1024 and root == (k == len(plan) - 1)
        at = hi
    assert at == n_rel


def test_edge_attr_dict_is_validated_before_any_work():
    g = torch.Generator().manual_seed(9)
    graph, n_in = hand_built(g)
    widths = {"a": 8, "b": 12}
    layer = make_layer(widths, [2, 2, 1], [4, 4, 8], True, [True, True, True], [3, None, 1])
    xs = {t: torch.randn((n_in[t], widths[t]), generator=g) for t in n_in}
    ea = edge_attrs(graph, layer, g)
    with pytest.raises(ValueError, match="edge_attr"):
        layer(xs, graph)                                                   # none at all
    with pytest.raises(ValueError, match="edge_attr"):
        layer(xs, graph, edge_attr_dict={ETS[0]: ea[ETS[0]]})              # a missing entry
    with pytest.raises(ValueError, match="shape"):
        layer(xs, graph, edge_attr_dict={**ea, ETS[0]: ea[ETS[0]][:, :2]})        # a wrong width
    with pytest.raises(ValueError, match="rows"):
        layer(xs, graph, edge_attr_dict={**ea, ETS[2]: ea[ETS[2]][:-1]})          # a wrong length
    with pytest.raises(NotImplementedError, match="edge_attr"):
        layer(xs, graph, edge_attr_dict={**ea, ETS[0]: ea[ETS[0]].clone().requires_grad_(True)})
    # over a dict of CSR pairs the entry goes to the relation as its edge_attr; a missing one is refused the same way
    csr = {r.edge_type: [r.row_ptr, r.col] for r in graph.relations}
    with pytest.raises(ValueError, match="edge_attr"):
        layer(xs, csr, edge_attr_dict={ETS[2]: ea[ETS[2]]})
