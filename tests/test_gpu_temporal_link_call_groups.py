"""GPU: TEMPORAL link call groups — ``LinkNeighborLoader(..., edge_label_time=..., time_attr=...)`` handed out by
``call_groups()`` (homogeneous) and ``hetero_call_groups()`` (typed edge seeds), the loop of the reference's movielens example.

* every mini-batch inside a group is bit for bit what ``for batch in loader`` yields (the one-batch-at-a-time temporal route, which
  ``for batch in loader`` keeps), on every store and key — homogeneous, heterogeneous with two endpoint types (``writes``) and with
  one (``cites``: a joint endpoint list), negatives None / binary 1.0 / binary 0.3 / triplet 2.0, with and without a node-level time
  attribute that gates the negatives, uniform and biased; groups of 4, then 2, then the ragged last batch;
* ``seed_time`` / ``seed_time_dict``: the time of a unique endpoint is that of the first pair of its mini-batch that names it
  (``link_loader._first_occurrence``);
* ``nn.HeteroConv`` of ``nn.SAGEConv`` over ``layer_graph(j)`` and ``nn.EdgeDecoder`` over the group's pairs against the same model
  over the per-batch objects in float64: seed rows within 1e-5 max|want| (the bar of tests/test_gpu_hetero_link_call_groups.py),
  the scores within that row tolerance carried through the decoder plus 1e-5 of the decoder's own magnitude sum;
* the refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 16
N_EDGES = 6 * B + 9                           # 6 full batches + one of 9; groups of 4 -> [4, 2, 1]
V = 500                                       # the homogeneous graph
N_P, N_A = 400, 150
HOMO = ("n", "e", "n")
CITES, WRITES, REV = ("paper", "cites", "paper"), ("author", "writes", "paper"), ("paper", "rev_writes", "author")
FAN = {CITES: [3, 2], WRITES: [2, 2], REV: [2, 1]}
F_IN, HIDDEN, OUT = {"paper": 8, "author": 4}, 16, 8
NEG = [None, ("binary", 1.0), ("binary", 0.3), ("triplet", 2.0)]
_STORES = {}


def _n_neg(neg, n_pos):
    from math import ceil
    return 0 if neg is None else max(int(ceil(neg[1] * n_pos)), 1)


def _stores(kind, node_time):
    """(feature store, graph store, {edge type: edges}) of the homogeneous / heterogeneous graph, with or without a node-level
    ``time``; edge times in [0, 100), strictly positive weights.  Built once and left unchanged."""
    key = (kind, node_time)
    if key not in _STORES:
        import torch
        from cugraph_pyg_amd.data import FeatureStore, GraphStore
        g = torch.Generator().manual_seed(41)
        gs, fs, edges = GraphStore(), FeatureStore(), {}
        shapes = {HOMO: (V, V, 5000)} if kind == "homo" else {CITES: (N_P, N_P, 3000), WRITES: (N_A, N_P, 1500), REV: (N_P, N_A, 1500)}
        for et, (n_src, n_dst, E) in shapes.items():
            ei = torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.randint(0, n_dst, (E,), generator=g)])
            if et == REV:
                ei = edges[WRITES].flip(0)
            edges[et] = ei
            gs[et, "coo", False, (n_src, n_dst)] = ei
            fs[et, "time", None] = torch.randint(0, 100, (E,), generator=g)
            fs[et, "w", None] = torch.rand(E, generator=g) + 0.05
        for t, n, f in ([("n", V, 8)] if kind == "homo" else [("paper", N_P, F_IN["paper"]), ("author", N_A, F_IN["author"])]):
            fs[t, "x", None] = torch.randn(n, f, generator=g)
            if node_time:       # when a node came into being: the negatives of a pair are redrawn until both ends exist at its time
                fs[t, "time", None] = torch.randint(0, 60, (n,), generator=g)
        _STORES[key] = (fs, gs, edges)
    return _STORES[key]


def _label_time():
    import torch
    return torch.randint(0, 100, (N_EDGES,), generator=torch.Generator().manual_seed(9))


def _loader(kind, neg, node_time=False, biased=False, per_call=4, **kw):
    import torch
    from cugraph_pyg_amd.loader import LinkNeighborLoader
    fs, gs, edges = _stores("homo" if kind == "homo" else "hetero", node_time)
    g = torch.Generator().manual_seed(7)
    et = HOMO if kind == "homo" else kind
    eli = edges[et][:, torch.randperm(edges[et].shape[1], generator=g)[:N_EDGES]]
    label = torch.randint(0, 2, (N_EDGES,), generator=g) if neg is None else None
    kw.setdefault("edge_label_time", _label_time())
    kw.setdefault("time_attr", "time")
    kw.setdefault("local_seeds_per_call", per_call * 2 * (B + _n_neg(neg, B)))
    return LinkNeighborLoader((fs, gs), kw.pop("fan", [3, 2] if kind == "homo" else FAN),
                              edge_label_index=eli if kind == "homo" else (et, eli), edge_label=label, batch_size=B, shuffle=False,
                              random_state=5, neg_sampling=neg, weight_attr="w" if biased else None, **kw)


def _same(a, b):
    import torch
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    return a == b


def _pair_times(input_id, n_pairs):
    """``t_all`` of a mini-batch: the positives' times, then negative k at the time of positive k mod n_pos."""
    import torch
    t_pos = _label_time().to(input_id.device)[input_id]
    n_pos = t_pos.numel()
    return torch.cat([t_pos, t_pos[torch.arange(n_pairs - n_pos, device=t_pos.device) % n_pos]])


@pytest.mark.parametrize("biased", [False, True], ids=["uniform", "biased"])
@pytest.mark.parametrize("node_time", [False, True], ids=["edge-times", "node-times"])
@pytest.mark.parametrize("neg", NEG, ids=["labels", "binary1", "binary0.3", "triplet2"])
def test_temporal_link_call_groups_equal_the_per_batch_loader(hiplib, neg, node_time, biased):
    import torch
    from cugraph_pyg_amd.loader.link_loader import _first_occurrence
    per_batch = list(_loader("homo", neg, node_time, biased))
    groups = list(_loader("homo", neg, node_time, biased).call_groups())
    assert [g.n_batches for g in groups] == [4, 2, 1] and len(per_batch) == 7
    assert sum(int(d.edge_index.shape[1]) for d in per_batch) > 0
    at = 0
    for g in groups:
        datas = g.to_data_list()
        assert len(datas) == g.n_batches
        bp = g.batch_ptr.tolist()
        assert g.seed_time.dtype == torch.int64 and g.seed_time.shape == (g.num_seeds,)
        for j, d in enumerate(datas):
            ref = per_batch[at + j]
            assert sorted(d.keys()) == sorted(ref.keys())
            for k in ref.keys():
                assert _same(d[k], ref[k]), (at + j, k)
            t_all = _pair_times(ref.input_id, ref.edge_label_index.shape[1])
            want = _first_occurrence(ref.edge_label_index.reshape(-1), torch.cat([t_all, t_all]), int(ref.num_sampled_nodes[0]))
            assert torch.equal(g.seed_time[bp[j]:bp[j + 1]], want), at + j
        at += g.n_batches
    assert at == 7


@pytest.mark.parametrize("biased", [False, True], ids=["uniform", "biased"])
@pytest.mark.parametrize("node_time", [False, True], ids=["edge-times", "node-times"])
@pytest.mark.parametrize("neg", NEG, ids=["labels", "binary1", "binary0.3", "triplet2"])
@pytest.mark.parametrize("etype", [WRITES, CITES], ids=["author-writes-paper", "paper-cites-paper"])
def test_temporal_hetero_link_call_groups_equal_the_per_batch_loader(hiplib, etype, neg, node_time, biased):
    import torch
    from cugraph_pyg_amd.loader.link_loader import _first_occurrence
    src_t, _, dst_t = etype
    seed_types = [src_t] if src_t == dst_t else [src_t, dst_t]
    per_batch = list(_loader(etype, neg, node_time, biased))
    groups = list(_loader(etype, neg, node_time, biased).hetero_call_groups())
    assert [g.n_batches for g in groups] == [4, 2, 1] and len(per_batch) == 7
    assert sum(int(d[et].edge_index.shape[1]) for d in per_batch for et in FAN) > 0
    at = 0
    for g in groups:
        datas = g.to_data_list()
        assert len(datas) == g.n_batches
        assert sorted(g.seed_time_dict) == sorted(seed_types)
        bp = {t: g.batch_ptr_dict[t].tolist() for t in seed_types}
        for j, d in enumerate(datas):
            ref = per_batch[at + j]
            assert sorted(map(str, d.node_types + d.edge_types)) == sorted(map(str, ref.node_types + ref.edge_types))
            for key in ref.node_types + ref.edge_types:
                assert sorted(d[key].keys()) == sorted(ref[key].keys()), key
                for k in ref[key].keys():
                    assert _same(d[key][k], ref[key][k]), (at + j, key, k)
            eli = ref[etype].edge_label_index
            t_all = _pair_times(ref[etype].input_id, eli.shape[1])
            if src_t == dst_t:
                want = {src_t: _first_occurrence(eli.reshape(-1), torch.cat([t_all, t_all]), int(ref[src_t].num_sampled_nodes[0]))}
            else:
                want = {src_t: _first_occurrence(eli[0], t_all, int(ref[src_t].num_sampled_nodes[0])),
                        dst_t: _first_occurrence(eli[1], t_all, int(ref[dst_t].num_sampled_nodes[0]))}
            for t in seed_types:
                got = g.seed_time_dict[t]
                assert got.dtype == torch.int64 and got.shape == (g.num_seeds_dict[t],)
                assert torch.equal(got[bp[t][j]:bp[t][j + 1]], want[t]), (at + j, t)
        at += g.n_batches
    assert at == 7


def _batch_rows(params, d, n_seed):
    """PyG's plain formulation on ONE heterogeneous mini-batch in float64: every layer over all sampled edges and all nodes —
    per edge type lin_l(mean over a node's in-edges) + bias + lin_r(the node's own row), summed over the edge types ending in
    the node's type, ReLU between the layers — and the first ``n_seed[t]`` rows (the seeds) of the result per type."""
    import torch
    h = {t: d[t].x.double() for t in F_IN}
    for j, layer in enumerate(params):
        out = {}
        for et, (wl, wr, b) in layer.items():
            src, dst = d[et].edge_index[0], d[et].edge_index[1]
            xs, xd = h[et[0]], h[et[2]]
            n = xd.shape[0]
            deg = torch.zeros(n, dtype=torch.float64, device=xd.device).index_add_(0, dst, torch.ones(dst.shape[0], dtype=torch.float64, device=xd.device))
            agg = torch.zeros((n, xs.shape[1]), dtype=torch.float64, device=xd.device).index_add(0, dst, xs[src]) / deg.clamp(min=1).unsqueeze(1)
            y = agg @ wl.t() + b + xd @ wr.t()
            out[et[2]] = y if et[2] not in out else out[et[2]] + y
        h = {t: torch.relu(y) for t, y in out.items()} if j + 1 < len(params) else out
    return {t: h[t][:n] for t, n in n_seed.items()}


def test_temporal_hetero_group_model_equals_the_per_batch_model(hiplib):
    import torch
    from wholegraph_amd import nn
    etype, neg = WRITES, ("binary", 2.0)
    src_t, _, dst_t = etype
    per_batch = list(_loader(etype, neg))
    groups = list(_loader(etype, neg).hetero_call_groups())
    torch.manual_seed(3)
    layers = [nn.HeteroConv({et: nn.SAGEConv((F_IN[et[0]], F_IN[et[2]]), HIDDEN) for et in FAN}).cuda(),
              nn.HeteroConv({et: nn.SAGEConv((HIDDEN, HIDDEN), OUT) for et in FAN}).cuda()]
    dec = nn.EdgeDecoder(HIDDEN, in_channels=(OUT, OUT)).cuda()
    params = [{et: tuple(p.detach().double() for p in (layer.conv(et).lin_l.weight, layer.conv(et).lin_r.weight, layer.conv(et).lin_l.bias))
               for et in FAN} for layer in layers]
    w1, b1, w2, b2 = (p.detach().double() for p in (dec.lin1.weight, dec.lin1.bias, dec.lin2.weight, dec.lin2.bias))
    at = 0
    with torch.no_grad():
        for g in groups:
            h = g.x_dict
            for j, layer in enumerate(layers):
                h = layer(h, g.layer_graph(j), act="relu" if j + 1 < len(layers) else None)
            scores = dec(h[src_t], h[dst_t], g.edge_label_index)
            bp = {t: g.batch_ptr_dict[t].tolist() for t in (src_t, dst_t)}
            lp = g.label_ptr.tolist()
            for j in range(g.n_batches):
                ref = per_batch[at + j]
                ns = {t: int(ref[t].num_sampled_nodes[0]) for t in (src_t, dst_t)}
                want = _batch_rows(params, ref, ns)
                tol = {}
                for t in (src_t, dst_t):
                    got = h[t][bp[t][j]:bp[t][j + 1]].double()
                    tol[t] = 1e-5 * (float(want[t].abs().max()) + 1e-30)
                    err = float((got - want[t]).abs().max())
                    print("batch %d %s rows: error %.3g bar %.3g" % (at + j, t, err, tol[t]))
                    assert err <= tol[t], (at + j, t, err, tol[t])
                i, k = ref[etype].edge_label_index
                z = torch.cat([want[src_t][i], want[dst_t][k]], -1)
                hid = z @ w1.t() + b1
                s64 = (torch.relu(hid) @ w2.t() + b2).view(-1)
                # the decoder's own rounding: 1e-5 of the magnitude sum of a score's terms; the rows' tolerance carried through it
                mag = ((z.abs() @ w1.abs().t() + b1.abs()) @ w2.abs().t() + b2.abs()).view(-1)
                carried = float((torch.cat([torch.full((OUT,), tol[src_t]), torch.full((OUT,), tol[dst_t])]).double().cuda()
                                 @ w1.abs().t() @ w2.abs().t()).view(-1)[0])
                err = (scores[lp[j]:lp[j + 1]].double() - s64).abs()
                bar = 1e-5 * mag + carried
                print("batch %d scores: worst error / bar %.3f" % (at + j, float((err / bar).max())))
                assert bool((err <= bar).all()), (at + j, float((err / bar).max()))
            at += g.n_batches
    assert at == 7


def test_temporal_link_call_groups_refusals(hiplib):
    import torch
    from cugraph_pyg_amd.loader import NeighborLoader
    t = _label_time()
    for kind, method in (("homo", "call_groups"), (WRITES, "hetero_call_groups")):
        fan_m1 = [-1, 2] if kind == "homo" else {CITES: [-1, 2], WRITES: [2, 2], REV: [2, 1]}
        fan_big = [300, 2] if kind == "homo" else {CITES: [300, 2], WRITES: [2, 2], REV: [2, 1]}
        for why, make in (
                ("temporal", lambda: _loader(kind, None, time_attr=None)),                       # edge_label_time without time_attr
                ("disjoint", lambda: _loader(kind, None, disjoint=True)),
                ("fan-out", lambda: _loader(kind, None, fan=fan_m1)),
                ("sampler-output", lambda: _loader(kind, None, as_sampler_output=True)),
                (r"temporal.*fan-outs 1\.\.256", lambda: _loader(kind, None, fan=fan_big))):     # outside temporal_call_groups_ok()
            with pytest.raises(NotImplementedError, match=why):
                getattr(make(), method)()
        with pytest.raises(NotImplementedError, match="replacement"):
            getattr(_loader(kind, None, replace=True, edge_label_time=None, time_attr=None), method)()
        # `for batch in loader` keeps the one-batch-at-a-time route: call_groups_ok() stays False for a temporal sampler
        groups = getattr(_loader(kind, None), method)()
        assert groups._smp.temporal and groups._smp.temporal_call_groups_ok() and not groups._smp.call_groups_ok()
        assert groups._smp.fetch_plan(N_EDGES, B)[0] == 0
    # a biased temporal loader whose weights are not strictly positive
    from cugraph_pyg_amd.data import FeatureStore, GraphStore
    ws, wf = GraphStore(), FeatureStore()
    ei = torch.stack([torch.arange(40), (torch.arange(40) + 5) % 50])
    ws[HOMO, "coo", False, (50, 50)] = ei
    wf[HOMO, "w", None] = torch.cat([torch.zeros(1), torch.ones(39)])
    wf[HOMO, "time", None] = torch.arange(40)
    wf["n", "x", None] = torch.randn(50, 4)
    from cugraph_pyg_amd.loader import LinkNeighborLoader
    zero_w = LinkNeighborLoader((wf, ws), [2, 2], edge_label_index=ei[:, :16], edge_label_time=torch.arange(16), time_attr="time",
                                weight_attr="w", batch_size=8)
    with pytest.raises(NotImplementedError, match="strictly positive"):
        zero_w.call_groups()
    # node seeds of a HETEROGENEOUS temporal graph stay refused
    fs, gs, _ = _stores("hetero", False)
    with pytest.raises(NotImplementedError):
        NeighborLoader((fs, gs), num_neighbors=FAN, batch_size=4, input_nodes=("paper", torch.arange(8)),
                       input_time=torch.full((8,), 50), time_attr="time").call_groups()
