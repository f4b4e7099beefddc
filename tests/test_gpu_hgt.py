"""wholegraph_amd.nn.HGTConv on the GPU against the float64 restatement (tests/hgt_ref.py): the one-launch layer kernel with its
joint softmax across relations, its two backward kernels, lazy inputs with row placement over two hops, the dict form, and the
torch route beyond eight relations.  Bars: forward |err| <= 1e-5 x magnitude sum + 1e-7 per element; gradients max |err| <= 1e-4 x
max |ref| per tensor, bitwise equal across two runs."""
import functools

import pytest

from hgt_ref import hgt_forward, layer_graph, params_of

pytestmark = pytest.mark.gpu
TYPES = ["a", "b"]
ETS = [("a", "r1", "a"), ("b", "r2", "a"), ("b", "r3", "a"), ("a", "r4", "b")]
N_IN, N_DST = {"a": 50, "b": 45}, 37       # 37 destinations per type: a partial last tile
# degrees of a's first rows in (r1, r2, r3): empty everywhere; the last relation only; one edge each; longer than any unroll next to
# 5; and the row whose largest logit lies in the second relation (p_rel = (1, 8, 1)), the rescale across the relation boundary
FIXED = [(0, 0, 0), (0, 0, 3), (1, 1, 1), (24, 5, 0), (2, 3, 1)]


def check_forward(got, ref, scale, what):
    for t in ref:
        err = (got[t].double() - ref[t]).abs()
        bar = 1e-5 * scale[t] + 1e-7
        print("%s %s: max |err| %.3e, max bar %.3e" % (what, t, float(err.max()), float(bar.max())))
        assert bool((err <= bar).all()), (what, t, float((err - bar).max()))


def check_grads(pairs):
    for name, got, want in pairs:
        if want is None:
            assert got is None or float(got.abs().max()) == 0.0, name
            continue
        err, ref = float((got.double() - want).abs().max()), float(want.abs().max())
        print("%s: max |err| %.3e, largest reference gradient %.3e" % (name, err, ref))
        assert err <= 1e-4 * ref, (name, err, ref)


@functools.lru_cache(maxsize=None)
def case(H, C, dev="cuda:0"):
    import torch
    from wholegraph_amd import nn
    g = torch.Generator().manual_seed(100 * H + C)
    torch.manual_seed(7 * H + C)
    conv = nn.HGTConv({"a": C, "b": C + 4}, C, (TYPES, ETS), heads=H).to(dev)
    with torch.no_grad():
        conv.p_rel["b__r2__a"].fill_(8.0)
        conv.skip["a"].fill_(0.4)
    x = {t: (torch.rand((N_IN[t], conv.in_channels[t]), generator=g) * 2 - 1).to(dev) for t in TYPES}
    edges = {}
    for k, et in enumerate(ETS):
        deg = torch.randint(0, 5, (N_DST,), generator=g)
        deg[0] = 0
        if et[2] == "a":
            deg[:len(FIXED)] = torch.tensor([f[k] for f in FIXED])
        dst = torch.repeat_interleave(torch.arange(N_DST), deg)
        edges[et] = (torch.randint(0, N_IN[et[0]], (int(deg.sum()),), generator=g), dst[torch.randperm(dst.shape[0], generator=g)])
    dst_rows = {t: torch.randperm(N_IN[t], generator=g)[:N_DST] for t in TYPES}
    graph = layer_graph(edges, dst_rows, TYPES, device=dev)
    x64, p64 = {t: v.double() for t, v in x.items()}, params_of(conv)
    refs = {relu: hgt_forward(x64, graph, p64, ETS, H, relu=relu, want_scale=True) for relu in (False, True)}
    return conv, x, graph, edges, dst_rows, refs


SHAPES = [(1, 4), (2, 24), (4, 64), (8, 256)]      # the smallest; three lanes per head; a power of two; the widest


@pytest.mark.parametrize("H,C", SHAPES)
@pytest.mark.parametrize("act", [None, "relu"])
def test_forward(hiplib, H, C, act):
    import torch
    from wholegraph_amd import nn
    conv, x, graph, _, _, refs = case(H, C)
    before = nn.hgt_launches
    with torch.no_grad():
        out = conv(x, graph, act=act)
    assert conv.route == "layer" and nn.hgt_launches - before == 2      # one launch per destination type, three relations in one
    check_forward(out, *refs[act == "relu"], "H %d C %d act %s" % (H, C, act))


def run_grads(conv, x, graph, gout, bitwise=True):
    """Every gradient of sum(out * gout); ``bitwise``: run twice, the same bits (the kernel route's claim: no atomics)."""
    import torch
    runs = []
    for _ in range(2 if bitwise else 1):
        for p in conv.parameters():
            p.grad = None
        xg = {t: v.clone().requires_grad_(True) for t, v in x.items()}
        out = conv(xg, graph, act="relu")
        sum((out[t] * gout[t]).sum() for t in out).backward()
        runs.append({**{k: p.grad for k, p in conv.named_parameters()}, **{"x." + t: v.grad for t, v in xg.items()}})
    assert all((runs[0][k] is None and runs[-1][k] is None) or torch.equal(runs[0][k], runs[-1][k]) for k in runs[0])
    return runs[0]


@pytest.mark.parametrize("H,C", SHAPES)
def test_gradients(hiplib, H, C):
    import torch
    from wholegraph_amd import nn
    conv, x, graph, _, _, _ = case(H, C)
    g = torch.Generator().manual_seed(C)
    gout = {t: (torch.rand((N_DST, C), generator=g) * 2 - 1).to(x[t].device) for t in TYPES}
    before = nn.hgt_launches
    got = run_grads(conv, x, graph, gout)
    assert conv.route == "layer" and nn.hgt_launches - before == 4
    p64 = {k: v.requires_grad_(True) for k, v in params_of(conv).items()}
    x64 = {t: v.double().requires_grad_(True) for t, v in x.items()}
    ref = hgt_forward(x64, graph, p64, ETS, H, relu=True)
    sum((ref[t] * gout[t].double()).sum() for t in ref).backward()
    check_grads([(k, got[k], p64[k].grad) for k in p64] + [("x." + t, got["x." + t], x64[t].grad) for t in TYPES])


def test_dict_form_is_the_layer_graph_result(hiplib):
    import torch
    conv, x, _, edges, _, _ = case(4, 64)
    with torch.no_grad():
        whole = {t: torch.arange(N_IN[t]) for t in TYPES}
        wide = {et: (s, d) for et, (s, d) in edges.items()}           # frontier entry d = input row d of the type here
        want = conv(x, layer_graph(wide, whole, TYPES, device=x["a"].device))
        got = conv(x, {et: torch.stack([s, d]).to(x["a"].device) for et, (s, d) in edges.items()})
    assert conv.route == "layer" and sorted(got) == sorted(want)
    assert all(torch.equal(got[t], want[t]) for t in want)


def test_nine_relations_take_the_torch_route(hiplib):
    import torch
    from wholegraph_amd import nn
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(9)
    ets = [("a", "r%d" % k, "a") for k in range(9)]
    torch.manual_seed(9)
    conv = nn.HGTConv(8, 8, (["a"], ets), heads=2).to(dev)
    x = {"a": (torch.rand((20, 8), generator=g) * 2 - 1).to(dev)}
    edges = {et: (torch.randint(0, 20, (30,), generator=g), torch.randint(0, 20, (30,), generator=g)) for et in ets}
    graph = layer_graph(edges, {"a": torch.arange(20)}, ["a"], device=dev)
    gout = {"a": (torch.rand((20, 8), generator=g) * 2 - 1).to(dev)}
    before = nn.hgt_launches
    with torch.no_grad():
        out = conv(x, graph, act="relu")
    assert conv.route == "torch" and nn.hgt_launches == before
    p64 = {k: v.requires_grad_(True) for k, v in params_of(conv).items()}
    x64 = {"a": x["a"].double().requires_grad_(True)}
    ref, scale = hgt_forward(x64, graph, p64, ets, 2, relu=True, want_scale=True)
    check_forward(out, {"a": ref["a"].detach()}, scale, "nine relations")
    got = run_grads(conv, x, graph, gout, bitwise=False)      # (torch's index_add: float atomics, no bitwise claim)
    (ref["a"] * gout["a"].double()).sum().backward()
    check_grads([(k, got[k], p64[k].grad) for k in p64] + [("x.a", got["x.a"], x64["a"].grad)])


def hetero_group():
    """Two node types, three edge types, fan-out [4, 3]: the first call group (as attr_group() of test_gpu_hetero_transformer.py)."""
    import torch
    from cugraph_pyg_amd.data import FeatureStore, GraphStore
    from cugraph_pyg_amd.loader import NeighborLoader
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(5)
    n = {"u": 2000, "v": 1500}
    ets = {("u", "to", "v"): 6000, ("v", "to", "u"): 5000, ("v", "self", "v"): 4000}
    gs, fs = GraphStore(), FeatureStore()
    for et, m in ets.items():
        gs[et, "coo", False, (n[et[0]], n[et[2]])] = torch.stack([torch.randint(0, n[et[0]], (m,), generator=g, device=dev),
                                                                  torch.randint(0, n[et[2]], (m,), generator=g, device=dev)])
    for t in n:
        fs[t, "x", None] = torch.rand((n[t], 32), generator=g, device=dev) * 2 - 1
    seeds = torch.randperm(n["v"], generator=g, device=dev)[:64 * 3]
    loader = NeighborLoader((fs, gs), {et: [4, 3] for et in ets}, input_nodes=("v", seeds), batch_size=64, shuffle=False,
                            random_state=3, local_seeds_per_call=64 * 3)
    return next(iter(loader.call_groups())), sorted(ets), dev


def test_two_hops_lazy_inputs_and_row_placement(hiplib):
    import torch
    from wholegraph_amd import nn
    grp, ets, dev = hetero_group()
    assert all(isinstance(v, nn.LazyRows) for v in grp.x_dict.values())
    torch.manual_seed(11)
    model = [nn.HGTConv(32, 32, (["u", "v"], ets), heads=4).to(dev), nn.HGTConv(32, 16, (["u", "v"], ets), heads=2).to(dev)]
    graphs = [grp.layer_graph(j) for j in range(2)]
    assert any(r.out_rows is not None for gr in graphs for r in gr.relations)
    runs = []
    for _ in range(2):
        for m in model:
            for p in m.parameters():
                p.grad = None
        before = nn.hgt_launches
        h = model[0](grp.x_dict, graphs[0], act="relu")
        out = model[1](h, graphs[1])
        assert all(m.route == "layer" for m in model) and nn.hgt_launches > before
        if not runs:
            gout = torch.rand(out["v"].shape, generator=torch.Generator().manual_seed(1)).to(dev) * 2 - 1
        (out["v"] * gout).sum().backward()
        runs.append([out["v"].detach()] + [p.grad for m in model for p in m.parameters()])
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(*runs))
    p64 = [{k: v.requires_grad_(True) for k, v in params_of(m).items()} for m in model]
    x64 = {t: v.materialize().double() for t, v in grp.x_dict.items()}
    h64 = hgt_forward(x64, graphs[0], p64[0], ets, 4, relu=True)
    ref, scale = hgt_forward(h64, graphs[1], p64[1], ets, 2, want_scale=True)
    check_forward({"v": runs[0][0]}, {"v": ref["v"].detach()}, scale, "two hops")
    (ref["v"] * gout.double()).sum().backward()
    check_grads([("layer %d %s" % (j, k), p.grad, p64[j][k].grad) for j, m in enumerate(model) for k, p in m.named_parameters()])
