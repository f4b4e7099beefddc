"""float64 restatement of torch_geometric.nn.HGTConv in plain index ops — the yardstick of the HGTConv tests, written from the
formula alone: per relation COO edges, k and v through the relation's head-wise maps, the edges of ALL relations into a type
concatenated, an explicit max-subtracted softmax per (destination, head), exact GELU, out_lin, the sigmoid gate.  The parameters
go by the layer's own state-dict names."""
import math

import torch


def params_of(conv):
    return {k: v.detach().double() for k, v in conv.named_parameters()}


def _coo(r):
    """(src row in the layer's input, frontier entry) of every edge of a relation hop."""
    deg = (r.row_ptr[1:] - r.row_ptr[:-1]).long()
    return r.col[:r.n_edges].long(), torch.repeat_interleave(torch.arange(r.n_rows, device=deg.device), deg)


def hgt_forward(x, graph, p, edge_types, H, relu=False, want_scale=False):
    """``out`` ({type: [n_out, C]}) of the layer over a ``HeteroLayerGraph`` — ``(out, scale)`` with ``want_scale``: the magnitude sum
    of each output element's terms (tests/gen_ref.py's convention for a layer of two products: the same chain over the absolute
    values of every input, weight and bias, the softmax weights as they are, |gelu(a)| <= |a|)."""
    mag = lambda v: v.detach().abs()      # noqa: E731
    C = p["k_rel.weight"].shape[1] * H
    D = C // H

    def kqv(t, which):
        w, b = p["kqv_lin.lins.%s.weight" % t][which * C:(which + 1) * C], p["kqv_lin.lins.%s.bias" % t][which * C:(which + 1) * C]
        return x[t] @ w.t() + b, mag(x[t]) @ mag(w).t() + mag(b)
    groups = {}
    for r in graph.relations:
        groups.setdefault((r.hop, r.edge_type[2]), []).append(r)
    out, scale = {}, {}
    for (_, dt), mine in sorted(groups.items(), key=lambda kv: kv[0]):
        head = mine[0]
        n = head.n_rows
        if n == 0:
            continue
        q = kqv(dt, 1)[0][head.dst_rows].view(n, H, D)
        logit, val, sval, dst = [], [], [], []
        for r in mine:
            if r.n_edges == 0:
                continue
            et = r.edge_type
            ri = edge_types.index(et)
            src, d = _coo(r)
            (k, _), (v, sv) = kqv(et[0], 0), kqv(et[0], 2)
            ka, va = p["k_rel.weight"][ri * H:(ri + 1) * H], p["v_rel.weight"][ri * H:(ri + 1) * H]
            kj = torch.einsum("ehd,hdf->ehf", k[src].view(-1, H, D), ka)
            logit.append((q[d] * kj).sum(-1) * p["p_rel." + "__".join(et)].view(1, H) / math.sqrt(D))
            val.append(torch.einsum("ehd,hdf->ehf", v[src].view(-1, H, D), va))
            sval.append(torch.einsum("ehd,hdf->ehf", sv[src].view(-1, H, D), mag(va)))
            dst.append(d)
        agg = torch.zeros((n, H, D), dtype=torch.float64, device=q.device)
        sagg = agg.clone()
        if logit:
            lg, v, sv, d = torch.cat(logit), torch.cat(val), torch.cat(sval), torch.cat(dst)
            top = torch.full((n, H), -math.inf, dtype=torch.float64, device=q.device)
            top = top.scatter_reduce(0, d.unsqueeze(1).expand(-1, H), lg.detach(), "amax")
            w = torch.exp(lg - top[d])
            den = torch.zeros((n, H), dtype=torch.float64, device=q.device).index_add(0, d, w)
            assert bool((den[torch.unique(d)] > 1e-30).all())
            alpha = w / den[d]
            agg, sagg = agg.index_add(0, d, alpha.unsqueeze(-1) * v), sagg.index_add(0, d, alpha.detach().unsqueeze(-1) * sv)
        wo, bo = p["out_lin.lins.%s.weight" % dt], p["out_lin.lins.%s.bias" % dt]
        o = torch.nn.functional.gelu(agg.reshape(n, C)) @ wo.t() + bo
        s = sagg.reshape(n, C) @ mag(wo).t() + mag(bo)
        if x[dt].shape[1] == C:
            g = torch.sigmoid(p["skip." + dt])
            o, s = g * o + (1 - g) * x[dt][head.dst_rows], g.detach() * s + (1 - g.detach()) * mag(x[dt][head.dst_rows])
        if relu:
            o = torch.relu(o)
        if dt not in out:
            out[dt] = torch.zeros((graph.n_out[dt], C), dtype=torch.float64, device=q.device)
            scale[dt] = torch.zeros_like(out[dt])
        rows = head.out_rows if head.out_rows is not None else torch.arange(n, device=q.device)
        out[dt], scale[dt] = out[dt].index_copy(0, rows, o), scale[dt].index_copy(0, rows, s)
    return (out, scale) if want_scale else out


def layer_graph(edges, dst_rows, node_types, out_rows=None, device="cpu"):
    """A one-hop ``HeteroLayerGraph`` from ``edges = {edge_type: (src row, frontier entry) int tensors}`` (stable sort on the entry)
    and ``dst_rows = {type: int64 [n]}``, the input row of every frontier entry of the type."""
    from wholegraph_amd.nn import HeteroLayerGraph, RelationHop
    rels = []
    for et, (src, dst) in edges.items():
        n = int(dst_rows[et[2]].shape[0])
        order = torch.sort(dst, stable=True).indices
        row_ptr = torch.zeros(n + 1, dtype=torch.int32)
        row_ptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n), 0)
        rels.append(RelationHop(et, 0, row_ptr.to(device), src[order].to(torch.int32).to(device), dst_rows[et[2]].to(device),
                                None if out_rows is None else out_rows[et[2]].to(device), int(src.shape[0]), 0))
    ends = {et[2] for et in edges}
    return HeteroLayerGraph(rels, {t: int(dst_rows[t].shape[0]) for t in ends}, node_types)
