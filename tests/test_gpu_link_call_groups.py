"""GPU: ``LinkNeighborLoader.call_groups()`` (cugraph_pyg_amd/loader/link_call_group.py) — an epoch of seed EDGES handed out
as block-diagonal call groups, with one ``edge_label_index`` over the seed rows of the last layer's output.

* every mini-batch inside a group is bit for bit what ``for batch in loader`` yields, on every key;
* ``batch[edge_label_index]`` are the batches' global endpoint ids back to back; ``label_ptr`` / ``input_id`` / ``edge_label`` match;
* ``overlap`` changes nothing;
* two ``nn.SAGEConv`` over ``layer_graph(j)`` (a walk over RAGGED per-batch seed lists) and ``nn.link_bce_with_logits`` equal the
  per-batch float64 formulation: seed rows within 1e-5 max|want|, the loss within the head's loss bar plus what that row
  tolerance can do to it, the weight gradients within 1e-5 x the magnitude sum of their terms."""
import numpy as np
import pytest

from test_gpu_call_group_loader import _model, _stores

pytestmark = pytest.mark.gpu

V, B, N_EDGES = 6000, 64, 9 * 64 + 17          # 9 full batches of 64 seed edges + one of 17


def _n_neg(neg, n_pos):
    from math import ceil
    return 0 if neg is None else max(int(ceil(neg[1] * n_pos)), 1)


def _loader(fs, gs, fanout, neg, per_call, **kw):
    import torch
    from cugraph_pyg_amd.loader import LinkNeighborLoader
    rng = np.random.default_rng(4)
    eli = torch.from_numpy(rng.integers(0, V, (2, N_EDGES)))
    label = torch.from_numpy(rng.integers(0, 2, N_EDGES)) if neg is None else None
    return LinkNeighborLoader((fs, gs), fanout, edge_label_index=eli, edge_label=label, batch_size=B, shuffle=False,
                              random_state=17, neg_sampling=neg, local_seeds_per_call=per_call * 2 * (B + _n_neg(neg, B)), **kw)


def _same(a, b):
    import torch
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    return a == b


def _batch_rows(params, d, masks, n_seed, magnitudes=False):
    """PyG's plain formulation on ONE mini-batch in float64 — every layer over all sampled edges and all nodes, mean over a
    node's in-edges, ReLU between the layers — and the seeds' rows of the result.  ``masks[j]`` (or None): the ReLU mask of the
    first rows of layer j's output, taken from the float32 forward (an element within round-off of the kink may have the other
    sign there, and the gradients would differ by that whole term).  ``magnitudes``: over |x| (``params`` are then magnitudes
    too): the magnitude sum of every term."""
    import torch
    x = d.x.double().abs() if magnitudes else d.x.double()
    src, dst = d.edge_index[0], d.edge_index[1]
    n = x.shape[0]
    deg = torch.zeros(n, dtype=torch.float64, device=x.device).index_add_(0, dst, torch.ones(dst.shape[0], dtype=torch.float64, device=x.device))
    h, used = x, []
    for j, (wl, wr, b) in enumerate(params):
        agg = torch.zeros((n, h.shape[1]), dtype=torch.float64, device=x.device).index_add(0, dst, h[src]) / deg.clamp(min=1).unsqueeze(1)
        h = agg @ wl.t() + b + h @ wr.t()
        if j + 1 < len(params):
            m = h.detach() > 0
            if masks is not None:
                m[:masks[j].shape[0]] = masks[j]
            used.append(m)
            h = h * m
    return h[:n_seed], used


NEG = [None, ("binary", 1.0), ("binary", 0.3), ("triplet", 2.0)]


@pytest.mark.parametrize("fanout,dims", [([5, 3], [32, 64, 16]), ([7], [32, 16])])
@pytest.mark.parametrize("per_call", [4, 1])
@pytest.mark.parametrize("neg", NEG, ids=["labels", "binary1", "binary0.3", "triplet2"])
def test_link_call_groups_equal_the_per_batch_loader_and_the_float64_formulation(hiplib, neg, per_call, fanout, dims):
    import torch
    import torch.nn.functional as F
    from wholegraph_amd import nn
    gs, fs, feat = _stores(V, 14, 32)
    per_batch = list(_loader(fs, gs, fanout, neg, per_call))
    groups = list(_loader(fs, gs, fanout, neg, per_call).call_groups())
    plain = list(_loader(fs, gs, fanout, neg, per_call).call_groups(overlap=False))
    assert [g.n_batches for g in groups] == ([4, 4, 1, 1] if per_call == 4 else [1] * 10) == [g.n_batches for g in plain]
    assert len(per_batch) == 10
    convs = _model(dims, "cuda")
    at = 0
    for g, q in zip(groups, plain):
        # ---- overlap or not: the same group -----------------------------------------------------------------------------
        assert torch.equal(g.n_id, q.n_id) and torch.equal(g.edge_label_index, q.edge_label_index)
        assert torch.equal(g.batch_ptr, q.batch_ptr) and torch.equal(g.node_ptr, q.node_ptr) and torch.equal(g.input_id, q.input_id)
        assert _same(g.edge_label, q.edge_label) and torch.equal(g.edge_index, q.edge_index) and torch.equal(g.e_id, q.e_id)
        # ---- every mini-batch of the group == the loader's own Data, on every key -------------------------------------------------
        datas = g.to_data_list()
        assert len(datas) == g.n_batches
        for j, d in enumerate(datas):
            ref = per_batch[at + j]
            assert sorted(d.keys()) == sorted(ref.keys())
            for k in ref.keys():
                assert _same(d[k], ref[k]), k
        refs = per_batch[at:at + g.n_batches]
        # ---- the group's pairs --------------------------------------------------------------------------------------------------
        n_pos = [r.batch_size for r in refs]
        n_pair = [r.edge_label_index.shape[1] for r in refs]
        assert g.label_ptr.tolist() == [0] + list(np.cumsum(n_pair)) and g.label_ptr.dtype == torch.int64
        assert g.edge_label_index.dtype == torch.int64 and g.edge_label_index.shape == (2, sum(n_pair))
        assert torch.equal(g.batch[g.edge_label_index], torch.cat([r.n_id[r.edge_label_index] for r in refs], 1))
        assert torch.equal(g.input_id, torch.cat([r.input_id for r in refs])) and g.input_id.numel() == sum(n_pos)
        assert _same(g.edge_label, torch.cat([r.edge_label for r in refs]))
        # ---- forward + loss + weight gradients against the per-batch float64 formulation ------------------------------------------
        for c in convs:
            for p in c.parameters():
                p.grad = None
        h, hidden = g.x, []
        for j, c in enumerate(convs):
            h = c(h, g.layer_graph(j), act="relu" if j + 1 < len(convs) else None)
            hidden.append(h)
        label = g.edge_label.float()
        loss = nn.link_bce_with_logits(h, h, g.edge_label_index, label)
        loss.backward()
        bp = g.batch_ptr.tolist()
        assert h.shape == (g.num_seeds, dims[-1]) and bp[-1] == g.num_seeds

        params = [tuple(p.detach().double().requires_grad_(True) for p in (c.lin_l.weight, c.lin_r.weight, c.lin_l.bias)) for c in convs]
        mags = [tuple(p.detach().abs().requires_grad_(True) for p in ps) for ps in params]
        rows64, rows_mag, hop0_at = [], [], 0
        for j, r in enumerate(refs):
            ns = int(r.num_sampled_nodes[0])
            assert ns == bp[j + 1] - bp[j]
            masks = None
            if len(convs) == 2:      # layer 0's output rows of this batch: its seeds, then the vertices its hop 0 found
                n1 = int(r.num_sampled_nodes[1])
                mine = torch.cat([hidden[0][bp[j]:bp[j + 1]], hidden[0][g.num_seeds + hop0_at:g.num_seeds + hop0_at + n1]])
                masks, hop0_at = [mine.detach() > 0], hop0_at + n1
            want, used = _batch_rows(params, r, masks, ns)
            got = h.detach()[bp[j]:bp[j + 1]].double()
            scale = float(want.detach().abs().max()) + 1e-30
            assert float((got - want.detach()).abs().max()) <= 1e-5 * scale, (j, float((got - want.detach()).abs().max()), scale)
            rows64.append(want)
            rows_mag.append(_batch_rows(mags, r, used, ns, magnitudes=True)[0])
        H, Ha = torch.cat(rows64), torch.cat(rows_mag)
        i, k = g.edge_label_index
        s = (H[i] * H[k]).sum(-1)
        loss64 = F.binary_cross_entropy_with_logits(s, label.double())
        loss64.backward()
        P = s.shape[0]
        M = (H.detach()[i] * H.detach()[k]).abs().sum(-1)
        delta = 1e-5 * float(H.detach().abs().max())         # what the rows' own tolerance may move a logit by, per unit of the other factor
        bar = 1e-5 * (float(M.mean()) + abs(float(loss64.detach()))) + delta * float((H.detach()[i].abs().sum(-1) + H.detach()[k].abs().sum(-1)).mean())
        got_loss, want_loss = float(loss.detach()), float(loss64.detach())
        print("loss %.9g ref %.9g error %.3g bar %.3g" % (got_loss, want_loss, abs(got_loss - want_loss), bar))
        assert abs(got_loss - want_loss) <= bar
        # magnitude sums: the same formulas over magnitudes, every pair weighted by |c_p| plus what a 1e-5 M_p error of its logit
        # does to the sigmoid
        Ma = (Ha.detach()[i] * Ha.detach()[k]).sum(-1)
        c_mag = (torch.sigmoid(s.detach()) - label.double()).abs() / P + 0.25 * Ma / P
        (c_mag * (Ha[i] * Ha[k]).sum(-1)).sum().backward()
        for c, ps, ms in zip(convs, params, mags):
            for got, want, mag, name in zip((c.lin_l.weight.grad, c.lin_r.weight.grad, c.lin_l.bias.grad), ps, ms, ("lin_l", "lin_r", "bias")):
                err = (got.double() - want.grad).abs()
                print("grad %s: worst error / bar %.3f" % (name, float((err / (1e-5 * mag.grad + 1e-300)).max())))
                assert bool((err <= 1e-5 * mag.grad).all()), (name, float((err / (1e-5 * mag.grad + 1e-300)).max()))
        at += g.n_batches
    assert at == 10


def test_link_call_groups_refuse_what_they_cannot_do(hiplib):
    import torch
    from cugraph_pyg_amd.data import FeatureStore, GraphStore
    from cugraph_pyg_amd.loader import LinkNeighborLoader
    gs, fs, _ = _stores(500, 6, 8)
    eli = torch.stack([torch.arange(64), torch.arange(64) + 7])
    kw = dict(edge_label_index=eli, batch_size=16)
    for why, loader in (
            ("temporal", lambda: LinkNeighborLoader((fs, gs), [3, 3], edge_label_time=torch.arange(64), **kw)),
            ("disjoint", lambda: LinkNeighborLoader((fs, gs), [3, 3], disjoint=True, **kw)),
            ("replacement", lambda: LinkNeighborLoader((fs, gs), [3, 3], replace=True, **kw)),
            ("fan-out", lambda: LinkNeighborLoader((fs, gs), [-1, 3], **kw)),
            ("sampler-output", lambda: LinkNeighborLoader((fs, gs), [3, 3], as_sampler_output=True, **kw))):
        with pytest.raises(NotImplementedError, match=why):
            loader().call_groups()
    hg, hf = GraphStore(), FeatureStore()
    hg[("paper", "cites", "paper"), "coo", False, (6, 6)] = [torch.tensor([0, 1, 2]), torch.tensor([1, 2, 3])]
    hg[("author", "writes", "paper"), "coo", False, (4, 6)] = [torch.tensor([0, 1, 2, 3]), torch.tensor([0, 1, 2, 3])]
    het = LinkNeighborLoader((hf, hg), {("paper", "cites", "paper"): [2], ("author", "writes", "paper"): [2]},
                             edge_label_index=(("author", "writes", "paper"), torch.tensor([[0, 1], [0, 1]])), batch_size=2)
    with pytest.raises(NotImplementedError, match="heterogeneous"):
        het.call_groups()
