"""GPU: ``LinkNeighborLoader.hetero_call_groups()`` (cugraph_pyg_amd/loader/link_call_group.py) — an epoch of typed seed EDGES of
a heterogeneous graph handed out as block-diagonal call groups, with one ``edge_label_index`` whose rows index the last layer's
output of the source and of the destination type.

* every mini-batch inside a group is bit for bit what ``for batch in loader`` yields, on every store and key;
* ``n_id[t][edge_label_index[i]]`` are the batches' global endpoint ids back to back; ``label_ptr`` / ``input_id`` / ``edge_label`` /
  ``batch_ptr_dict`` match the per-batch objects; ``overlap`` changes nothing;
* two ``nn.HeteroConv`` of ``nn.SAGEConv`` over ``layer_graph(j)`` (a walk over RAGGED per-batch seed lists of two node types) and
  ``nn.link_bce_with_logits(h[src_t], h[dst_t], ...)`` equal the per-batch float64 plain formulation — every layer over all
  sampled edges of the batch's ``HeteroData``, then the seeds' rows — at the bars of tests/test_gpu_link_call_groups.py: seed rows
  within 1e-5 max|want|, the loss within the head's loss bar plus what that row tolerance can do to it, the weight gradients
  within 1e-5 x the magnitude sum of their terms (ReLU masks from the float32 forward)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_P, N_A, B = 2500, 900, 40                   # the graph of test_hetero_link_loader_call_groups_equal_one_batch_path
N_EDGES = 6 * B + 9                           # 6 full batches + one of 9; groups of 4 -> [4, 2, 1]
CITES, WRITES, REV = ("paper", "cites", "paper"), ("author", "writes", "paper"), ("paper", "rev_writes", "author")
FAN = {CITES: [3, 2], WRITES: [2, 2], REV: [2, 1]}
F_IN, HIDDEN, OUT = {"paper": 8, "author": 4}, 16, 8
NEG = [None, ("binary", 1.0), ("binary", 0.3), ("triplet", 2.0)]
_GRAPH = {}


def _n_neg(neg, n_pos):
    from math import ceil
    return 0 if neg is None else max(int(ceil(neg[1] * n_pos)), 1)


def _stores():
    """(feature store, graph store, {edge type: its edges}) — built once and left unchanged."""
    if not _GRAPH:
        import torch
        from cugraph_pyg_amd.data import FeatureStore, GraphStore
        g = torch.Generator().manual_seed(33)
        cites = torch.stack([torch.randint(0, N_P, (15000,), generator=g), torch.randint(0, N_P, (15000,), generator=g)])
        writes = torch.stack([torch.randint(0, N_A, (7000,), generator=g), torch.randint(0, N_P, (7000,), generator=g)])
        gs, fs = GraphStore(), FeatureStore()
        gs[CITES, "coo", False, (N_P, N_P)] = cites
        gs[WRITES, "coo", False, (N_A, N_P)] = writes
        gs[REV, "coo", False, (N_P, N_A)] = writes.flip(0)
        fs["paper", "x", None] = torch.randn(N_P, F_IN["paper"], generator=g)
        fs["author", "x", None] = torch.randn(N_A, F_IN["author"], generator=g)
        fs[WRITES, "w", None] = torch.randn(7000, 2, generator=g)
        _GRAPH["v"] = (fs, gs, {CITES: cites, WRITES: writes})
    return _GRAPH["v"]


def _loader(etype, neg, per_call=4, **kw):
    import torch
    from cugraph_pyg_amd.loader import LinkNeighborLoader
    fs, gs, edges = _stores()
    g = torch.Generator().manual_seed(7)
    eli = edges[etype][:, torch.randperm(edges[etype].shape[1], generator=g)[:N_EDGES]]
    label = torch.randint(0, 2, (N_EDGES,), generator=g) if neg is None else None
    kw.setdefault("local_seeds_per_call", per_call * 2 * (B + _n_neg(neg, B)))
    return LinkNeighborLoader((fs, gs), kw.pop("fan", FAN), edge_label_index=(etype, eli), edge_label=label, batch_size=B, shuffle=False,
                              random_state=5, neg_sampling=neg, **kw)


def _same(a, b):
    import torch
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    return a == b


def _model(dev):
    import torch
    from wholegraph_amd import nn
    torch.manual_seed(3)
    return [nn.HeteroConv({et: nn.SAGEConv((F_IN[et[0]], F_IN[et[2]]), HIDDEN) for et in FAN}).to(dev),
            nn.HeteroConv({et: nn.SAGEConv((HIDDEN, HIDDEN), OUT) for et in FAN}).to(dev)]


def _batch_rows(params, d, masks, n_seed, magnitudes=False):
    """PyG's plain formulation on ONE heterogeneous mini-batch in float64: every layer over all sampled edges and all nodes —
    per edge type lin_l(mean over a node's in-edges) + bias + lin_r(the node's own row), summed over the edge types ending in
    the node's type, ReLU between the layers — and the first ``n_seed[t]`` rows (the seeds) of the result per type.
    ``masks[j]`` (or None): {type: the ReLU mask of the first rows of layer j's output, from the float32 forward};
    ``magnitudes``: over |x| (``params`` are then magnitudes too): the magnitude sum of every term."""
    import torch
    h = {t: (d[t].x.double().abs() if magnitudes else d[t].x.double()) for t in F_IN}
    used = []
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
        if j + 1 < len(params):
            ms = {}
            for t, y in out.items():
                m = y.detach() > 0
                if masks is not None:
                    m[:masks[j][t].shape[0]] = masks[j][t]
                ms[t] = m
                out[t] = y * m
            used.append(ms)
        h = out
    return {t: h[t][:n] for t, n in n_seed.items()}, used


@pytest.mark.parametrize("etype", [WRITES, CITES], ids=["author-writes-paper", "paper-cites-paper"])
@pytest.mark.parametrize("neg", NEG, ids=["labels", "binary1", "binary0.3", "triplet2"])
def test_hetero_link_call_groups_equal_the_per_batch_loader_and_the_float64_formulation(hiplib, neg, etype):
    import torch
    import torch.nn.functional as F
    from wholegraph_amd import nn
    src_t, _, dst_t = etype
    seed_types = [src_t] if src_t == dst_t else [src_t, dst_t]
    per_batch = list(_loader(etype, neg))
    groups = list(_loader(etype, neg).hetero_call_groups())
    plain = list(_loader(etype, neg).hetero_call_groups(overlap=False))
    assert [g.n_batches for g in groups] == [4, 2, 1] == [g.n_batches for g in plain]
    assert len(per_batch) == 7
    layers = _model("cuda")
    at = 0
    for g, q in zip(groups, plain):
        assert g.edge_type == etype and g.seed_types == (src_t, dst_t) and g.seed_type == src_t
        # ---- overlap or not: the same group -----------------------------------------------------------------------------
        for t in F_IN:
            assert torch.equal(g.n_id[t], q.n_id[t]) and torch.equal(g.node_ptr[t], q.node_ptr[t])
        assert torch.equal(g.edge_label_index, q.edge_label_index) and torch.equal(g.input_id, q.input_id)
        assert _same(g.edge_label, q.edge_label) and torch.equal(g.label_ptr, q.label_ptr) and torch.equal(g.batch_ptr, q.batch_ptr)
        assert sorted(g.batch_ptr_dict) == sorted(seed_types) == sorted(q.batch_ptr_dict)
        assert all(torch.equal(g.batch_ptr_dict[t], q.batch_ptr_dict[t]) for t in seed_types)
        assert g.num_sampled_nodes == q.num_sampled_nodes and g.num_sampled_edges == q.num_sampled_edges
        # ---- every mini-batch of the group == the loader's own HeteroData, on every store and key ----------------------------------
        datas = g.to_data_list()
        assert len(datas) == g.n_batches
        refs = per_batch[at:at + g.n_batches]
        for d, ref in zip(datas, refs):
            stores = sorted(map(str, ref.node_types + ref.edge_types))
            assert sorted(map(str, d.node_types + d.edge_types)) == stores
            for key in ref.node_types + ref.edge_types:
                assert sorted(d[key].keys()) == sorted(ref[key].keys()), key
                for k in ref[key].keys():
                    assert _same(d[key][k], ref[key][k]), (key, k)
            if neg is not None and neg[0] == "triplet":
                assert {"src_index", "dst_pos_index", "dst_neg_index"} <= set(d[etype].keys())
        # ---- the group's pairs --------------------------------------------------------------------------------------------------
        n_pos = [r[etype].batch_size for r in refs]
        n_pair = [r[etype].edge_label_index.shape[1] for r in refs]
        assert g.n_pos == n_pos[0] and g.n_pos + g.n_neg == n_pair[0]
        assert g.label_ptr.tolist() == [0] + list(np.cumsum(n_pair)) and g.label_ptr.dtype == torch.int64
        assert g.edge_label_index.dtype == torch.int64 and g.edge_label_index.shape == (2, sum(n_pair))
        assert torch.equal(g.n_id[src_t][_seed_rows(g, src_t)[g.edge_label_index[0]]],
                           torch.cat([r[src_t].n_id[r[etype].edge_label_index[0]] for r in refs]))
        assert torch.equal(g.n_id[dst_t][_seed_rows(g, dst_t)[g.edge_label_index[1]]],
                           torch.cat([r[dst_t].n_id[r[etype].edge_label_index[1]] for r in refs]))
        assert torch.equal(g.input_id, torch.cat([r[etype].input_id for r in refs])) and g.input_id.numel() == sum(n_pos)
        assert _same(g.edge_label, torch.cat([r[etype].edge_label for r in refs]))
        for t in seed_types:
            sizes = [int(r[t].num_sampled_nodes[0]) for r in refs]
            assert g.batch_ptr_dict[t].dtype == torch.int32 and g.batch_ptr_dict[t].tolist() == [0] + list(np.cumsum(sizes))
            assert g.num_seeds_dict[t] == sum(sizes)
        assert torch.equal(g.batch_ptr, g.batch_ptr_dict[src_t]) and g.num_seeds == g.num_seeds_dict[src_t]
        # ---- forward + loss + weight gradients against the per-batch float64 formulation ------------------------------------------
        for layer in layers:
            for p in layer.parameters():
                p.grad = None
        h, hidden = g.x_dict, []
        for j, layer in enumerate(layers):
            h = layer(h, g.layer_graph(j), act="relu" if j + 1 < len(layers) else None)
            hidden.append(h)
        label = g.edge_label.float()
        loss = nn.link_bce_with_logits(h[src_t], h[dst_t], g.edge_label_index, label)
        loss.backward()
        bp = {t: g.batch_ptr_dict[t].tolist() for t in seed_types}
        for t in seed_types:
            assert h[t].shape == (g.num_seeds_dict[t], OUT)
        lvl1 = {t: g._seg(1, t, False).tolist() for t in F_IN}       # per-batch rows of layer 0's output: the batch's seeds + hop-0 finds

        def leaves(f):
            return [{et: tuple(f(p) for p in (layer.conv(et).lin_l.weight, layer.conv(et).lin_r.weight, layer.conv(et).lin_l.bias))
                     for et in FAN} for layer in layers]
        params = leaves(lambda p: p.detach().double().requires_grad_(True))
        mags = leaves(lambda p: p.detach().abs().double().requires_grad_(True))
        rows64, rows_mag = {t: [] for t in seed_types}, {t: [] for t in seed_types}
        for j, r in enumerate(refs):
            ns = {t: int(r[t].num_sampled_nodes[0]) for t in seed_types}
            masks = [{t: hidden[0][t][lvl1[t][j]:lvl1[t][j + 1]].detach() > 0 for t in hidden[0]}]
            for t in masks[0]:
                assert masks[0][t].shape[0] == int(r[t].num_sampled_nodes[0]) + int(r[t].num_sampled_nodes[1])
            want, used = _batch_rows(params, r, masks, ns)
            mag, _ = _batch_rows(mags, r, used, ns, magnitudes=True)
            for t in seed_types:
                got = h[t].detach()[bp[t][j]:bp[t][j + 1]].double()
                scale = float(want[t].detach().abs().max()) + 1e-30
                err = float((got - want[t].detach()).abs().max())
                assert err <= 1e-5 * scale, (t, j, err, scale)
                rows64[t].append(want[t])
                rows_mag[t].append(mag[t])
        H = {t: torch.cat(rows64[t]) for t in seed_types}
        Ha = {t: torch.cat(rows_mag[t]) for t in seed_types}
        i, k = g.edge_label_index
        Hs, Hd, Has, Had = H[src_t], H[dst_t], Ha[src_t], Ha[dst_t]
        s = (Hs[i] * Hd[k]).sum(-1)
        loss64 = F.binary_cross_entropy_with_logits(s, label.double())
        loss64.backward()
        P = s.shape[0]
        M = (Hs.detach()[i] * Hd.detach()[k]).abs().sum(-1)
        # what the rows' own tolerance may move a logit by, per unit of the other factor
        d_src, d_dst = 1e-5 * float(Hs.detach().abs().max()), 1e-5 * float(Hd.detach().abs().max())
        bar = 1e-5 * (float(M.mean()) + abs(float(loss64.detach()))) + float(
            (d_dst * Hs.detach()[i].abs().sum(-1) + d_src * Hd.detach()[k].abs().sum(-1)).mean())
        got_loss, want_loss = float(loss.detach()), float(loss64.detach())
        print("loss %.9g ref %.9g error %.3g bar %.3g" % (got_loss, want_loss, abs(got_loss - want_loss), bar))
        assert abs(got_loss - want_loss) <= bar
        Ma = (Has.detach()[i] * Had.detach()[k]).sum(-1)
        c_mag = (torch.sigmoid(s.detach()) - label.double()).abs() / P + 0.25 * Ma / P
        (c_mag * (Has[i] * Had[k]).sum(-1)).sum().backward()
        checked = 0
        for layer, ps, ms in zip(layers, params, mags):
            for et in FAN:
                c = layer.conv(et)
                for got, want, mag, name in zip((c.lin_l.weight.grad, c.lin_r.weight.grad, c.lin_l.bias.grad), ps[et], ms[et],
                                                ("lin_l", "lin_r", "bias")):
                    if want.grad is None:       # a relation the seed types never reach in this layer
                        assert got is None or float(got.abs().max()) == 0.0, (et, name)
                        continue
                    err = (got.double() - want.grad).abs()
                    worst = float((err / (1e-5 * mag.grad + 1e-300)).max())
                    print("grad %s %s: worst error / bar %.3f" % (et[1], name, worst))
                    assert bool((err <= 1e-5 * mag.grad).all()), (et, name, worst)
                    checked += 1
        assert checked >= 9
        at += g.n_batches
    assert at == 7


def _seed_rows(g, t):
    """Rows of the group's level-0 vertices of type ``t`` (``batch_ptr_dict`` numbering) in ``n_id[t]``: every mini-batch's
    vertex list starts with its seeds."""
    import torch
    ptr, bp = g.node_ptr[t].long(), g.batch_ptr_dict[t].long()
    G = g.n_batches
    per = bp[1:G + 1] - bp[:G]
    start = torch.repeat_interleave(ptr[:G], per)
    within = torch.arange(int(bp[G]), device=ptr.device) - torch.repeat_interleave(bp[:G], per)
    return start + within


def test_hetero_link_call_groups_refuse_what_they_cannot_do(hiplib):
    import torch
    from cugraph_pyg_amd.data import FeatureStore, GraphStore
    from cugraph_pyg_amd.loader import LinkNeighborLoader
    fs, gs, edges = _stores()
    for why, loader in (
            ("temporal", lambda: _loader(WRITES, None, edge_label_time=torch.arange(N_EDGES))),
            ("disjoint", lambda: _loader(WRITES, None, disjoint=True)),
            ("replacement", lambda: _loader(WRITES, None, replace=True)),
            ("fan-out", lambda: _loader(WRITES, None, fan={CITES: [-1, 2], WRITES: [2, 2], REV: [2, 1]})),
            ("sampler-output", lambda: _loader(WRITES, None, as_sampler_output=True))):
        with pytest.raises(NotImplementedError, match=why):
            loader().hetero_call_groups()
    ws, wf = GraphStore(), FeatureStore()       # biased sampling with a weight that is not strictly positive: call_groups_ok() is false
    ws[CITES, "coo", False, (N_P, N_P)] = edges[CITES][:, :200]
    wf[CITES, "wt", None] = torch.cat([torch.zeros(1), torch.ones(199)])
    biased = LinkNeighborLoader((wf, ws), {CITES: [2]}, edge_label_index=(CITES, edges[CITES][:, :16]), batch_size=8, weight_attr="wt")
    with pytest.raises(NotImplementedError, match="sampler configuration"):
        biased.hetero_call_groups()
    # the wrong method on either kind of graph names the right one
    with pytest.raises(NotImplementedError, match=r"heterogeneous.*hetero_call_groups\(\)"):
        _loader(WRITES, None).call_groups()
    hs, hf = GraphStore(), FeatureStore()
    hs[("n", "e", "n"), "coo", False, (50, 50)] = [torch.arange(40), torch.arange(40) + 5]
    hf["n", "x", None] = torch.randn(50, 4)
    homo = LinkNeighborLoader((hf, hs), [2, 2], edge_label_index=torch.stack([torch.arange(32), torch.arange(32) + 3]), batch_size=8)
    with pytest.raises(NotImplementedError, match=r"homogeneous.*call_groups\(\)"):
        homo.hetero_call_groups()
