"""nn.HeteroConv over SAGEConv relations on the GPU: one wgamd_hetero_sage_layer_f32 launch per (hop, destination type) of a call
group (split into consecutive launches where the stacked row is wider than 1024 floats), forward and backward, against the float64
restatement of tests/hetero_sage_ref.py.  Bars: forward — every element within 1e-5 x the magnitude sum of its terms
(sum |c_k w_k| + |b|: the project's bar for fp32 layers); gradients — within 1e-4 x the largest reference gradient of the tensor
(the TransformerConv bar), and bitwise equal from run to run.  Every test checks through ``nn.hetero_sage_launches`` that the
kernel route ran."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)


def mag_group(F_in, seed=9):
    """A small ogbn-mag-like call group (the node / relation counts of test_hetero_conv_trains_aggregate_first_...)."""
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
    return grp, etypes, dev, g


def sage_model(etypes, widths, dev, seed=0, **kw):
    import torch
    from wholegraph_amd import nn
    torch.manual_seed(seed)
    return [nn.HeteroConv({et: nn.SAGEConv((fin, fin), fout, **kw) for et in etypes}).to(dev) for fin, fout in widths]


def expected_launches(layer, graph):
    from wholegraph_amd import nn
    total, seen = 0, set()
    for r in graph.relations:
        key = (r.hop, r.edge_type[2])
        if key in seen or r.n_rows == 0:
            continue
        seen.add(key)
        convs = [layer.conv(et) for et in layer.edge_types if et[2] == key[1]]
        roots = [c.lin_r.weight.shape[1] for c in convs if c.lin_r is not None]
        total += len(nn.hetero_sage_plan([c.lin_l.weight.shape[1] for c in convs], roots[0] if roots else 0))
    return total


def check_forward(layer, xs, graph, out, relu, tag):
    """``out`` against float64 over the same inputs, element by element at 1e-5 x the magnitude sum of the element's terms."""
    import hetero_sage_ref as ref
    p = ref.params_of(layer)
    x = {t: (v.materialize() if hasattr(v, "materialize") else v).detach() for t, v in xs.items()}
    want = ref.hetero_sage_forward(x, graph, p, relu=relu)
    mag = ref.hetero_sage_forward(x, graph, p, abs_terms=True)
    assert set(out) == set(want), (tag, sorted(out), sorted(want))
    for t in want:
        err = (out[t].detach().double() - want[t]).abs()
        worst = float((err / mag[t].clamp(min=1e-30)).max())
        print("%s %s: max |err| %.3e, worst err / magnitude sum %.3e" % (tag, t, float(err.max()), worst))
        assert bool((err <= 1e-5 * mag[t]).all()), (tag, t, worst)


@pytest.mark.parametrize("F_in,hidden", [(128, 128), (100, 64), (128, 256)])
def test_two_layers_forward_match_float64_lazy_and_resident(hiplib, F_in, hidden):
    import torch
    from wholegraph_amd import nn
    grp, etypes, dev, g = mag_group(F_in)
    model = sage_model(etypes, [(F_in, hidden), (hidden, hidden)], dev)
    with torch.no_grad():
        outs = {}
        for resident in (None, "author", "paper"):
            h = {t: (v.materialize() if t == resident else v) for t, v in grp.x_dict.items()}
            for j, layer in enumerate(model):
                graph = grp.layer_graph(j)
                before = nn.hetero_sage_launches
                h_in, h = h, layer(h, graph, act="relu")
                assert nn.hetero_sage_launches - before == expected_launches(layer, graph), "the kernel route did not run"
                if resident is None:
                    check_forward(layer, h_in, graph, h, True, "F_in %d hidden %d layer %d" % (F_in, hidden, j))
            outs[resident] = h["paper"]
        assert outs[None].shape == (128 * 4, hidden)
        assert torch.equal(outs[None], outs["author"]) and torch.equal(outs[None], outs["paper"])
    if hidden == 256:      # paper at layer 1: four relation blocks and the root, 1280 floats: two launches
        convs = [model[1].conv(et) for et in model[1].edge_types if et[2] == "paper"]
        assert len(nn.hetero_sage_plan([c.lin_l.weight.shape[1] for c in convs], 256)) == 2


def test_gradients_match_float64_and_repeat_bit_for_bit(hiplib):
    """Two layers without ReLU (a pre-activation within rounding of zero would flip rows between two formulations), one node
    type resident and requiring a gradient, the others lazy."""
    import torch
    import hetero_sage_ref as ref
    from wholegraph_amd import nn
    F_in, hidden = 128, 128
    grp, etypes, dev, g = mag_group(F_in)
    model = sage_model(etypes, [(F_in, hidden), (hidden, hidden)], dev)
    params = [p for m in model for p in m.parameters()]
    gout = torch.randn((128 * 4, hidden), generator=g, device=dev)
    x_paper = grp.x_dict["paper"].materialize().clone()
    runs = []
    for _ in range(2):
        for p in params:
            p.grad = None
        xp = x_paper.clone().requires_grad_(True)
        h = {t: (xp if t == "paper" else v) for t, v in grp.x_dict.items()}
        before = nn.hetero_sage_launches
        for j, layer in enumerate(model):
            h = layer(h, grp.layer_graph(j), act=None)
        assert nn.hetero_sage_launches - before == sum(expected_launches(m, grp.layer_graph(j)) for j, m in enumerate(model))
        h["paper"].backward(gout)
        assert nn.hetero_sage_launches - before > sum(expected_launches(m, grp.layer_graph(j)) for j, m in enumerate(model)), \
            "the input gradient did not run on the layer kernel"
        runs.append((h["paper"].detach().clone(), [None if p.grad is None else p.grad.clone() for p in params], xp.grad.clone()))
    (o1, g1, gx1), (o2, g2, gx2) = runs
    assert torch.equal(o1, o2) and torch.equal(gx1, gx2)
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(g1, g2))
    # float64: the restatement under autograd from gout back to every parameter and the resident input
    x64 = {t: v.materialize().double() for t, v in grp.x_dict.items()}
    x64["paper"] = x_paper.double().requires_grad_(True)
    leaves, h = [], x64
    for j, layer in enumerate(model):
        p64 = ref.params_of(layer)
        for et in layer.edge_types:
            c = layer.conv(et)
            for k, q in (("Wl", c.lin_l.weight), ("bl", c.lin_l.bias), ("Wr", None if c.lin_r is None else c.lin_r.weight)):
                if q is not None:
                    p64[et][k] = p64[et][k].double().requires_grad_(True)
                    leaves.append((q, p64[et][k], (j, et, k)))
        h = ref.hetero_sage_forward(h, grp.layer_graph(j), p64)
    h["paper"].backward(gout.double())
    assert float((o1.double() - h["paper"].detach()).abs().max()) <= 2e-5 * float(h["paper"].detach().abs().max())
    used = 0
    for q, leaf, name in leaves:
        if leaf.grad is None:       # (a relation the seeds' type never reaches in the last layer)
            assert q.grad is None or float(q.grad.abs().max()) == 0.0, name
            continue
        used += 1
        scale = float(leaf.grad.abs().max())
        err = float((q.grad.double() - leaf.grad).abs().max())
        print("%s: max |err| %.3e, largest reference gradient %.3e" % (name, err, scale))
        assert err <= 1e-4 * scale, (name, err, scale)
    assert used >= 20
    scale = float(x64["paper"].grad.abs().max())
    err = float((gx1.double() - x64["paper"].grad).abs().max())
    print("x[paper]: max |err| %.3e, largest reference gradient %.3e" % (err, scale))
    assert err <= 1e-4 * scale


def test_second_backward_raises_and_a_fresh_pass_repeats_the_gradients(hiplib):
    """The kept C rows of a group are released by the first backward pass whatever retain_graph says: a second backward raises
    a RuntimeError that says so, and a fresh forward and backward gives the first pass's gradients bit for bit."""
    import torch
    from wholegraph_amd import nn
    grp, etypes, dev, g = mag_group(64)
    (layer,) = sage_model(etypes, [(64, 64)], dev)
    params = list(layer.parameters())
    xp = grp.x_dict["paper"].materialize().clone().requires_grad_(True)
    xs = {t: (xp if t == "paper" else v) for t, v in grp.x_dict.items()}
    graph = grp.layer_graph(0)

    def loss():
        before = nn.hetero_sage_launches
        out = layer(xs, graph, act="relu")
        assert nn.hetero_sage_launches - before == expected_launches(layer, graph), "the kernel route did not run"
        return sum(v.sum() for v in out.values())
    total = loss()
    total.backward(retain_graph=True)
    reached = {r.edge_type[2] for r in graph.relations if r.n_rows > 0}      # (a type no hop ends in launches nothing)
    assert xp.grad is not None and "paper" in reached
    assert all(p.grad is not None for et in layer.edge_types if et[2] in reached for p in layer.conv(et).parameters())
    first = [None if t.grad is None else t.grad.clone() for t in [xp] + params]
    with pytest.raises(RuntimeError, match="a second time"):
        total.backward()
    for t in [xp] + params:
        t.grad = None
    loss().backward()
    for t, want in zip([xp] + params, first):
        assert (t.grad is None and want is None) or torch.equal(t.grad, want)


def random_csr(n_rows, n_src, max_deg, g, dev):
    import torch
    deg = torch.randint(0, max_deg + 1, (n_rows,), generator=g, device=dev) if max_deg > 0 else torch.zeros(n_rows, dtype=torch.int64, device=dev)
    rp = torch.zeros(n_rows + 1, dtype=torch.int32, device=dev)
    rp[1:] = torch.cumsum(deg, 0).to(torch.int32)
    col = torch.randint(0, n_src, (int(rp[-1]),), generator=g, device=dev).to(torch.int32)
    return rp, col


def test_bipartite_widths_interleaved_placement_empty_hop_and_empty_type(hiplib):
    """A hand-built layer graph: a bipartite pair with F_src != F_dst plus a self relation; two hops of one type writing
    interleaved output rows; a hop in which no relation sampled an edge (its rows are act(root + bias)); a type with zero
    frontier rows (no launch); root_weight=False and aggr="sum" on one relation each; under autograd too."""
    import torch
    from wholegraph_amd import nn
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(4)
    n_in = {"u": 700, "v": 900, "w": 50}
    width = {"u": 64, "v": 96, "w": 32}
    ets = [("u", "r", "v"), ("v", "r", "u"), ("v", "s", "v"), ("w", "r", "w")]
    perm = torch.randperm(500, generator=g, device=dev)
    rows_h0, rows_h1, rows_h2 = perm[:150].contiguous(), perm[150:460].contiguous(), perm[460:].contiguous()   # interleaved rows of v
    dst_v = torch.randperm(n_in["v"], generator=g, device=dev)
    rels = []
    at = 0
    for hop, rows, deg in ((0, rows_h0, 6), (1, rows_h1, 12), (2, rows_h2, 0)):      # hop 2 of v: no relation sampled an edge
        n = int(rows.shape[0])
        dst = dst_v[at:at + n].contiguous()
        at += n
        for et in (ets[0], ets[2]):
            rp, col = random_csr(n, n_in[et[0]], deg, g, dev)
            rels.append(nn.RelationHop(et, hop, rp, col, dst, rows, int(col.shape[0]), max(deg, 1)))
    n_u = 333
    rp, col = random_csr(n_u, n_in["v"], 9, g, dev)
    rels.append(nn.RelationHop(ets[1], 1, rp, col, torch.randperm(n_in["u"], generator=g, device=dev)[:n_u].contiguous(),
                               torch.randperm(n_u, generator=g, device=dev), int(col.shape[0]), 9))
    rp0 = torch.zeros(1, dtype=torch.int32, device=dev)
    rels.append(nn.RelationHop(ets[3], 1, rp0, torch.zeros(0, dtype=torch.int32, device=dev),
                               torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev), 0, 1))
    graph = nn.HeteroLayerGraph(rels, {"u": n_u, "v": 500, "w": 0}, ["u", "v", "w"])
    torch.manual_seed(3)
    layer = nn.HeteroConv({
        ets[0]: nn.SAGEConv((64, 96), 72, aggr="sum"), ets[1]: nn.SAGEConv((96, 64), 72),
        ets[2]: nn.SAGEConv((96, 96), 72, root_weight=False), ets[3]: nn.SAGEConv((32, 32), 72)}).to(dev)
    xs = {t: torch.randn((n_in[t], width[t]), generator=g, device=dev) for t in n_in}
    for relu in (False, True):
        with torch.no_grad():
            before = nn.hetero_sage_launches
            out = layer(xs, graph, act="relu" if relu else None)
            assert nn.hetero_sage_launches - before == 4          # v: three hops, u: one; w has no frontier rows: no launch
        assert set(out) == {"u", "v"}
        check_forward(layer, xs, graph, out, relu, "hand-built relu=%s" % relu)
        # hop 2 of v: act(root + bias), the sum of both relations' biases and the one root weight
        c0, c2 = layer.conv(ets[0]), layer.conv(ets[2])
        want = xs["v"][dst_v[460:500]].double() @ c0.lin_r.weight.double().t() + c0.lin_l.bias.double() + c2.lin_l.bias.double()
        want = torch.relu(want) if relu else want
        assert float((out["v"][rows_h2].detach().double() - want.detach()).abs().max()) <= 1e-5 * float(want.abs().max() + 1)
    # under autograd: same outputs as the inference launches, bit for bit
    out_t = layer(xs, graph, act="relu")
    assert out_t["v"].requires_grad and torch.equal(out_t["v"].detach(), out["v"]) and torch.equal(out_t["u"].detach(), out["u"])


def test_shapes_outside_the_kernel_domain_take_library_ops(hiplib):
    import torch
    from wholegraph_amd import nn
    grp, etypes, dev, g = mag_group(30)           # F % 4 != 0
    model = sage_model(etypes, [(30, 24)], dev)
    before = nn.hetero_sage_launches
    with torch.no_grad():
        h = model[0](grp.x_dict, grp.layer_graph(0), act="relu")
    assert nn.hetero_sage_launches == before
    check_forward(model[0], grp.x_dict, grp.layer_graph(0), h, True, "library ops F=30")


def test_hetero_sage_call_groups_example_learns(hiplib, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import hetero_sage_call_groups as ex
    from wholegraph_amd import nn
    monkeypatch.setattr(sys, "argv", ["x", "--items", "20000", "--users", "10000", "--epochs", "6", "--batch-size", "256", "--group", "4"])
    before = nn.hetero_sage_launches
    loss, acc = ex.main()
    assert nn.hetero_sage_launches > before
    assert loss < 1.0 and acc > 0.7, (loss, acc)    # chance: ln 8 = 2.08, 1 / 8
