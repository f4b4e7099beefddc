"""nn.HeteroConv over TransformerConv relations on the GPU: one wgamd_hetero_transformer_layer_f32 launch per (hop, destination
type) of a call group (split into consecutive launches where the stacked row is wider than 1024 floats), forward and backward,
against the float64 restatement of tests/hetero_transformer_ref.py.  Bars: forward — every element within 1e-5 x the magnitude
sum of its terms (the project's bar for fp32 layers); gradients — within 1e-4 x the largest reference gradient of the tensor
(the TransformerConv bar; lin_key.bias, whose true gradient is zero because it cancels in the softmax, against lin_key.weight's
scale), and bitwise equal from run to run.  Every kernel-route test checks through ``nn.hetero_transformer_launches`` that the
kernel route ran."""
import functools
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

NAMES = {"Wq": ("lin_query", "weight"), "bq": ("lin_query", "bias"), "Wk": ("lin_key", "weight"), "bk": ("lin_key", "bias"),
         "Wv": ("lin_value", "weight"), "bv": ("lin_value", "bias"), "We": ("lin_edge", "weight"), "Ws": ("lin_skip", "weight"),
         "bs": ("lin_skip", "bias")}


@functools.lru_cache(maxsize=None)
def mag_group(F_in, seed=9):
    """A small ogbn-mag-like call group (the helper of tests/test_gpu_hetero_sage.py, re-created): made once per width."""
    import torch
    import bench_mag as bm
    dev = torch.device("cuda", 0)
    nodes = {"paper": 3000, "author": 4000, "institution": 200, "field_of_study": 500}
    rels = {k: max(v // 400, 1500) for k, v in bm.MAG_RELS.items()}
    graphs, num_nodes = bm.build_mag_like(dev, nodes, rels, seed=seed)
    etypes, ntypes = sorted(graphs), sorted(num_nodes)
    g = torch.Generator(device=dev).manual_seed(2)
    tables = {t: torch.rand((num_nodes[t], F_in), generator=g, device=dev) * 2 - 1 for t in ntypes}
    B, G = 128, 4
    seeds = torch.randperm(num_nodes["paper"], generator=g, device=dev)[:B * G]
    grp = next(iter(bm.make_loader(bm.build_mag_like.graph_store, tables, seeds, B, G).call_groups()))
    return grp, etypes, dev


@functools.lru_cache(maxsize=None)
def attr_group():
    """A small heterogeneous GraphStore + FeatureStore with an edge attribute ``attr = [src_id, dst_id]`` (floats, ids < 2^24):
    two node types, three edge types, a few thousand edges each -> its first call group."""
    import torch
    from cugraph_pyg_amd.data import FeatureStore, GraphStore
    from cugraph_pyg_amd.loader import NeighborLoader
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(5)
    n = {"u": 2000, "v": 1500}
    ets = {("u", "to", "v"): 6000, ("v", "to", "u"): 5000, ("v", "self", "v"): 4000}
    gs, fs = GraphStore(), FeatureStore()
    for et, m in ets.items():
        ei = torch.stack([torch.randint(0, n[et[0]], (m,), generator=g, device=dev), torch.randint(0, n[et[2]], (m,), generator=g, device=dev)])
        gs[et, "coo", False, (n[et[0]], n[et[2]])] = ei
        fs[et, "attr", None] = ei.t().float().contiguous()
    for t in n:
        fs[t, "x", None] = torch.rand((n[t], 32), generator=g, device=dev) * 2 - 1
    seeds = torch.randperm(n["v"], generator=g, device=dev)[:64 * 3]
    loader = NeighborLoader((fs, gs), {et: [4, 3] for et in ets}, input_nodes=("v", seeds), batch_size=64, shuffle=False,
                            random_state=3, local_seeds_per_call=64 * 3)
    return next(iter(loader.call_groups())), sorted(ets), dev


def tconv_model(etypes, widths, dev, seed=0, **kw):
    import torch
    from wholegraph_amd import nn
    torch.manual_seed(seed)
    return [nn.HeteroConv({et: nn.TransformerConv((fin, fin), fout, **kw) for et in etypes}).to(dev) for fin, fout in widths]


def expected_launches(layer, graph, xs):
    from wholegraph_amd import nn
    total, seen = 0, set()
    for r in graph.relations:
        key = (r.hop, r.edge_type[2])
        if key in seen or r.n_rows == 0:
            continue
        seen.add(key)
        convs = [layer.conv(et) for et in layer.edge_types if et[2] == key[1] and et[0] in xs]
        widths = [c.heads * nn.transformer_block_width(c.in_src, c.edge_dim or 0) for c in convs]
        total += len(nn.hetero_sage_plan(widths, convs[0].in_dst if any(c.root_weight for c in convs) else 0))
    return total


def dense(xs):
    return {t: (v.materialize() if hasattr(v, "materialize") else v).detach() for t, v in xs.items()}


def check_forward(layer, xs, graph, out, relu, tag, ea=None, rows=None):
    """``out`` against float64 over the same inputs, element by element at 1e-5 x the magnitude sum of the element's terms
    (``rows``: {type: the output rows to compare}, all by default)."""
    import hetero_transformer_ref as ref
    p, x = ref.params_of(layer), dense(xs)
    want = ref.hetero_transformer_forward(x, graph, p, ea, relu=relu)
    mag = ref.hetero_transformer_forward(x, graph, p, ea, abs_terms=True)
    assert set(out) == set(want), (tag, sorted(out), sorted(want))
    for t in want:
        sel = slice(None) if rows is None else rows[t]
        err = (out[t].detach().double() - want[t]).abs()[sel]
        worst = float((err / mag[t][sel].clamp(min=1e-30)).max())
        print("%s %s: max |err| %.3e, worst err / magnitude sum %.3e" % (tag, t, float(err.max()), worst))
        assert bool((err <= 1e-5 * mag[t][sel]).all()), (tag, t, worst)


ETS = [("a", "r1", "a"), ("b", "r2", "a"), ("b", "r3", "a")]


def hand_built(dev, g):
    """37 destination rows (two full tiles plus 5), three relations into type ``a``; per-relation degrees cycle through 0, 1, 3,
    4, 5, 9, 17 (the group-of-4 boundaries), offset per relation; rows 20 and 36 have no edge in any relation, row 8 edges in r2
    alone, row 9 in r1 alone; out_rows a permutation into a 50-row output.  (``hand_layer``: r1 F 64, H 2, D 3; r2 F 36, H 2,
    no edge_dim; r3 F 36, H 1, D 1; out_channels 16, 16, 32 with concat=True — three outputs 32 wide — and 32 each with
    concat=False, where the width is out_channels itself and the relations, being summed, must agree on it.)"""
    import torch
    from wholegraph_amd import nn
    n_in, n = {"a": 60, "b": 45}, 37
    cyc = [0, 1, 3, 4, 5, 9, 17]
    dst = torch.randperm(n_in["a"], generator=g, device=dev)[:n].contiguous()
    rows = torch.randperm(50, generator=g, device=dev)[:n].contiguous()
    rels = []
    for k, et in enumerate(ETS):
        deg = [cyc[(i + 2 * k) % 7] for i in range(n)]
        for i in (20, 36):
            deg[i] = 0
        if k != 1:
            deg[8] = 0
        if k != 0:
            deg[9] = 0
        rp = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        rp[1:] = torch.cumsum(torch.tensor(deg, device=dev), 0).to(torch.int32)
        col = torch.randint(0, n_in[et[0]], (int(rp[-1]),), generator=g, device=dev).to(torch.int32)
        rels.append(nn.RelationHop(et, 0, rp, col, dst, rows, int(rp[-1]), 17))
    assert rels[1].row_ptr[9] - rels[1].row_ptr[8] > 0 and rels[0].row_ptr[10] - rels[0].row_ptr[9] > 0
    return nn.HeteroLayerGraph(rels, {"a": 50, "b": 0}, ["a", "b"]), n_in, rows


def hand_layer(dev, concat, F_b=36, seed=1):
    import torch
    from wholegraph_amd import nn
    torch.manual_seed(seed)
    H, C, D = [2, 2, 1], ([16, 16, 32] if concat else [32, 32, 32]), [3, None, 1]
    F_ = {"a": 64, "b": F_b}
    return nn.HeteroConv({et: nn.TransformerConv((F_[et[0]], 64), C[k], heads=H[k], concat=concat, edge_dim=D[k])
                          for k, et in enumerate(ETS)}).to(dev)


@pytest.mark.parametrize("concat", [True, False])
def test_hand_built_group_relu_placement_sentinel_and_alpha(hiplib, concat):
    import torch
    from wholegraph_amd import nn
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(4)
    graph, n_in, rows = hand_built(dev, g)
    layer = hand_layer(dev, concat)
    xs = {"a": torch.randn((60, 64), generator=g, device=dev), "b": torch.randn((45, 36), generator=g, device=dev)}
    ea = {r.edge_type: torch.randn((r.n_edges, layer.conv(r.edge_type).edge_dim), generator=g, device=dev)
          for r in graph.relations if layer.conv(r.edge_type).edge_dim is not None}
    outs = {}
    for relu in (False, True):
        with torch.no_grad():
            before = nn.hetero_transformer_launches
            out = layer(xs, graph, act="relu" if relu else None, edge_attr_dict=ea)
            assert nn.hetero_transformer_launches - before == 1, "the kernel route did not run"
        assert set(out) == {"a"} and out["a"].shape == (50, 32)
        check_forward(layer, xs, graph, out, relu, "hand-built concat=%s relu=%s" % (concat, relu), ea=ea, rows={"a": rows})
        outs[relu] = out["a"]
    # the launch itself: a 50-row output pre-filled with a sentinel keeps it in the rows out_rows does not name; the _train form
    # gives the same bits, and every relation's alpha sums to 1 per (row, head) where the row has edges
    with torch.no_grad():
        wt, bias, fold, fold_b, layout = layer._tconv_weights(ETS)
        uw = torch.addmm(fold_b, xs["a"][graph.relations[0].dst_rows], fold)
        rels, alphas = [], []
        for r, lay in zip(graph.relations, layout):
            a = ea.get(r.edge_type)
            u = uw[:, lay["u0"]:lay["u0"] + lay["H"] * lay["F"]]
            w = uw[:, lay["w0"]:lay["w0"] + lay["H"] * lay["D"]] if lay["D"] else None
            alphas.append(torch.full((r.n_edges, lay["H"]), 7.0, device=dev))
            rels.append((r.row_ptr, r.col, xs[r.edge_type[0]], None, a, u, w, lay["H"], alphas[-1]))
        root = (xs["a"], graph.relations[0].dst_rows, None)
        for train in (False, True):
            target = torch.full((50, 32), -123.0, device=dev)
            A = torch.empty((37, wt.shape[1]), device=dev) if train else None
            nn.hetero_transformer_launch([t if train else t[:8] + (None,) for t in rels], 37, wt, 32, root=root, bias=bias, relu=True,
                                         out_rows=rows, out=target, a_save=A)
            assert torch.equal(target[rows], outs[True][rows])
            untouched = torch.ones(50, dtype=torch.bool, device=dev)
            untouched[rows] = False
            assert int(untouched.sum()) == 13 and bool((target[untouched] == -123.0).all())
        for r, lay, al in zip(graph.relations, layout, alphas):
            deg = (r.row_ptr[1:] - r.row_ptr[:-1]).long()
            row = torch.repeat_interleave(torch.arange(37, device=dev), deg)
            sums = torch.zeros((37, lay["H"]), device=dev).index_add(0, row, al)
            assert float((sums[deg > 0] - 1).abs().max()) <= 1e-5 and float(sums[deg == 0].abs().max()) == 0.0
            # a row without edges in the relation: the relation's blocks of A are exactly zero
            blk = A[:, lay["col0"]:lay["col0"] + lay["width"]]
            assert float(blk[deg == 0].abs().max()) == 0.0
            assert bool((blk[deg > 0][:, lay["F"] + lay["D"]] - 1).abs().max() <= 1e-5)      # the "1" column: sum alpha


def two_layers(grp, model, resident, act, ea=None, check=None):
    from wholegraph_amd import nn
    h = {t: (v.materialize() if t == resident else v) for t, v in grp.x_dict.items()}
    for j, layer in enumerate(model):
        graph = grp.layer_graph(j)
        before = nn.hetero_transformer_launches
        h_in, h = h, layer(h, graph, act=act, edge_attr_dict=ea)
        assert nn.hetero_transformer_launches - before == expected_launches(layer, graph, h_in), "the kernel route did not run"
        if check is not None:
            check_forward(layer, h_in, graph, h, act == "relu", "%s layer %d" % (check, j), ea=ea)
    return h


@pytest.mark.parametrize("F_in,hidden", [(128, 64), (256, 256)])
def test_two_layers_forward_match_float64_lazy_and_resident(hiplib, F_in, hidden):
    import torch
    from wholegraph_amd import nn
    grp, etypes, dev = mag_group(F_in)
    model = tconv_model(etypes, [(F_in, hidden), (hidden, hidden)], dev, heads=1, concat=False)
    with torch.no_grad():
        outs = {}
        for resident in (None, "author", "paper"):
            h = two_layers(grp, model, resident, "relu", check="F_in %d hidden %d" % (F_in, hidden) if resident is None else None)
            outs[resident] = h["paper"]
        assert outs[None].shape == (128 * 4, hidden)
        assert torch.equal(outs[None], outs["author"]) and torch.equal(outs[None], outs["paper"])
    if hidden == 256:      # paper at layer 1: four relation blocks of 260 and the 256 root, 1296 floats: two launches
        convs = [model[1].conv(et) for et in model[1].edge_types if et[2] == "paper"]
        widths = [c.heads * nn.transformer_block_width(c.in_src, 0) for c in convs]
        assert widths == [260] * 4
        plan = nn.hetero_sage_plan(widths, 256, max_k=nn.HETERO_TRANSFORMER_MAX_K)
        assert plan == [(0, 3, False), (3, 4, True)]


def test_edge_attributes_through_the_loader(hiplib):
    import torch
    grp, etypes, dev = attr_group()
    attr = grp.edge_attr("attr")
    assert set(attr) == set(etypes)
    n_id = grp.n_id
    graph = grp.layer_graph(0)
    seen = 0
    for r in graph.relations:
        if r.n_edges == 0:
            continue
        s_t, _, d_t = r.edge_type
        deg = (r.row_ptr[1:] - r.row_ptr[:-1]).long()
        row = torch.repeat_interleave(torch.arange(r.n_rows, device=dev), deg)
        want = torch.stack([n_id[s_t][r.col.long()[:r.n_edges]], n_id[d_t][r.dst_rows[row]]], 1).float()
        assert torch.equal(attr[r.edge_type][r.edge_base:r.edge_base + r.n_edges], want), r.edge_type
        seen += r.n_edges
    assert seen == sum(int(v.shape[0]) for v in attr.values()) == graph.num_edges > 1000
    assert all(int(attr[et].shape[0]) == graph.num_group_edges[et] for et in etypes)
    # two edge_dim = 2 layers (the ids scaled by a power of two: logits of order 1, a softmax that is not one-hot)
    ea = {et: v / 1024 for et, v in attr.items()}
    model = tconv_model(etypes, [(32, 32), (32, 32)], dev, heads=2, concat=False, edge_dim=2)
    with torch.no_grad():
        h = two_layers(grp, model, None, "relu", ea=ea, check="edge_dim 2")
    assert h["v"].shape == (64 * 3, 32)


def gradients_against_float64(grp, model, t_res, ea, gout, min_used):
    import torch
    import hetero_transformer_ref as ref
    params = [p for m in model for p in m.parameters()]
    x_res = grp.x_dict[t_res].materialize().clone()
    runs = []
    for _ in range(2):
        for p in params:
            p.grad = None
        xp = x_res.clone().requires_grad_(True)
        h = {t: (xp if t == t_res else v) for t, v in grp.x_dict.items()}
        for j, layer in enumerate(model):
            from wholegraph_amd import nn
            graph = grp.layer_graph(j)
            before = nn.hetero_transformer_launches
            n_want = expected_launches(layer, graph, h)
            h = layer(h, graph, act=None, edge_attr_dict=ea)
            assert nn.hetero_transformer_launches - before == n_want, "the kernel route did not run"
        h[t_res].backward(gout)
        runs.append((h[t_res].detach().clone(), [None if p.grad is None else p.grad.clone() for p in params], xp.grad.clone()))
    (o1, g1, gx1), (o2, g2, gx2) = runs
    assert torch.equal(o1, o2) and torch.equal(gx1, gx2)
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(g1, g2))
    # float64: the restatement under autograd from gout back to every parameter and the resident input
    x64 = {t: v.materialize().double() for t, v in grp.x_dict.items()}
    x64[t_res] = x_res.double().requires_grad_(True)
    ea64 = None if ea is None else {et: v.double() for et, v in ea.items()}
    leaves, h = [], x64
    for j, layer in enumerate(model):
        p64 = ref.params_of(layer)
        for et in layer.edge_types:
            c = layer.conv(et)
            for k, (mod, name) in NAMES.items():
                if p64[et]["p"].get(k) is not None:
                    p64[et]["p"][k] = p64[et]["p"][k].double().requires_grad_(True)
                    leaves.append((getattr(getattr(c, mod), name), p64[et]["p"][k], (j, et, k), c))
        h = ref.hetero_transformer_forward(h, grp.layer_graph(j), p64, ea64)
    h[t_res].backward(gout.double())
    assert float((o1.double() - h[t_res].detach()).abs().max()) <= 2e-5 * float(h[t_res].detach().abs().max())
    used = 0
    for q, leaf, name, c in leaves:
        if leaf.grad is None:       # (a relation the seeds' type never reaches in the last layer, or one without edges)
            assert q.grad is None or float(q.grad.abs().max()) == 0.0, name
            continue
        if name[2] == "bk":         # cancels in the softmax: zero, on the scale of lin_key.weight's gradient
            assert float(q.grad.abs().max()) <= 1e-4 * float(c.lin_key.weight.grad.abs().max()), name
            continue
        used += 1
        scale = float(leaf.grad.abs().max())
        err = float((q.grad.double() - leaf.grad).abs().max())
        print("%s: max |err| %.3e, largest reference gradient %.3e" % (name, err, scale))
        assert err <= 1e-4 * scale, (name, err, scale)
    assert used >= min_used, used
    scale = float(x64[t_res].grad.abs().max())
    err = float((gx1.double() - x64[t_res].grad).abs().max())
    print("x[%s]: max |err| %.3e, largest reference gradient %.3e" % (t_res, err, scale))
    assert err <= 1e-4 * scale


def test_gradients_match_float64_and_repeat_bit_for_bit(hiplib):
    """Two layers without ReLU (a pre-activation within rounding of zero would flip rows between two formulations), one node
    type resident and requiring a gradient, the others lazy."""
    import torch
    grp, etypes, dev = mag_group(128)
    model = tconv_model(etypes, [(128, 64), (64, 64)], dev, heads=1, concat=False)
    g = torch.Generator(device=dev).manual_seed(8)
    gradients_against_float64(grp, model, "paper", None, torch.randn((128 * 4, 64), generator=g, device=dev), 40)


def test_gradients_with_edge_attributes(hiplib):
    import torch
    grp, etypes, dev = attr_group()
    ea = {et: v / 1024 for et, v in grp.edge_attr("attr").items()}
    model = tconv_model(etypes, [(32, 32), (32, 32)], dev, seed=2, heads=2, concat=False, edge_dim=2)
    g = torch.Generator(device=dev).manual_seed(6)
    gradients_against_float64(grp, model, "v", ea, torch.randn((64 * 3, 32), generator=g, device=dev), 30)


def test_shapes_outside_the_kernel_domain_take_library_ops(hiplib):
    """A relation with F_src = 30 (not a multiple of 4): the whole layer runs library ops, matches float64, no launch."""
    import torch
    from wholegraph_amd import nn
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(4)
    graph, n_in, rows = hand_built(dev, g)
    layer = hand_layer(dev, True, F_b=30)
    xs = {"a": torch.randn((60, 64), generator=g, device=dev), "b": torch.randn((45, 30), generator=g, device=dev)}
    ea = {r.edge_type: torch.randn((r.n_edges, layer.conv(r.edge_type).edge_dim), generator=g, device=dev)
          for r in graph.relations if layer.conv(r.edge_type).edge_dim is not None}
    before = nn.hetero_transformer_launches
    with torch.no_grad():
        out = layer(xs, graph, act="relu", edge_attr_dict=ea)
    assert nn.hetero_transformer_launches == before
    check_forward(layer, xs, graph, out, True, "library ops F=30", ea=ea)


@pytest.mark.parametrize("torch_ops", [False, True])
def test_hetero_transformer_call_groups_example_learns(hiplib, monkeypatch, torch_ops):
    """A few call groups of examples/hetero_transformer_call_groups.py on either route: the loss falls and held-out items are
    classified far above chance (1 / 8)."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import hetero_transformer_call_groups as ex
    from wholegraph_amd import nn
    monkeypatch.setattr(sys, "argv", ["x", "--items", "20000", "--users", "10000", "--epochs", "2", "--batch-size", "256", "--group", "4",
                                      "--max-groups", "8"] + (["--torch-ops"] if torch_ops else []))
    before = nn.hetero_transformer_launches
    loss, acc = ex.main()
    assert (nn.hetero_transformer_launches > before) != torch_ops
    assert loss < 1.5 and acc > 0.4, (loss, acc)    # chance: ln 8 = 2.08, 1 / 8
