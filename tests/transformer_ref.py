"""float64 restatement of torch_geometric.nn.TransformerConv (flow source_to_target, beta=False, no dropout) — the yardstick of
the TransformerConv tests.  For edge j -> i and head h: q_i = lin_query(x_dst_i), k_j = lin_key(x_j), v_j = lin_value(x_j),
e_ij = lin_edge(edge_attr_ij) (edge_dim only; added to k_j and v_j), alpha = softmax over the edges into i of
q_i . k_j / sqrt(C) (PyG's softmax: exp(s - max) / (sum + 1e-16)), out_i = sum_j alpha v_j, heads concatenated or averaged,
plus lin_skip(x_dst_i) with root_weight.  A destination without edges gets the skip term alone.  Loops and duplicate edges are
ordinary edges."""
import math

import torch


def _lin(x, w, b=None):
    y = x @ w.double().t()
    return y if b is None else y + b.double()


def params_of(conv):
    """The parameters of a TransformerConv (or anything with PyG's names) as a dict of detached tensors."""
    d = lambda m, k: None if m is None or getattr(m, k, None) is None else getattr(m, k).detach()   # noqa: E731
    return dict(Wq=d(conv.lin_query, "weight"), bq=d(conv.lin_query, "bias"), Wk=d(conv.lin_key, "weight"),
                bk=d(conv.lin_key, "bias"), Wv=d(conv.lin_value, "weight"), bv=d(conv.lin_value, "bias"),
                We=d(conv.lin_edge, "weight"), Ws=d(conv.lin_skip, "weight") if conv.root_weight else None,
                bs=d(conv.lin_skip, "bias") if conv.root_weight else None)


def transformer_forward(x_src, x_dst, edge_index, p, heads, concat=True, edge_attr=None, relu=False, abs_terms=False,
                        return_alpha=False):
    """PyG TransformerConv in float64 over x_dst's rows (``x_dst`` None: x_src's).  ``p``: ``params_of(conv)`` (tensors may
    require grad).  ``abs_terms``: the magnitude sum of the output's terms — sum_j alpha (|Wv| |x_j| + |bv| + |We| |a_ij|) per
    head (alpha the true weights, averaged like the output) + |Ws| |x_dst_i| + |bs| — the scale of the accuracy bar."""
    dev = x_src.device
    xs = x_src.double()
    xd = xs if x_dst is None else x_dst.double()
    src = torch.as_tensor(edge_index[0]).long().to(dev)
    dst = torch.as_tensor(edge_index[1]).long().to(dev)
    n, E, H = xd.shape[0], src.shape[0], heads
    C = p["Wq"].shape[0] // H
    q = _lin(xd, p["Wq"], p["bq"]).view(n, H, C)
    k = _lin(xs[src], p["Wk"], p["bk"]).view(E, H, C)
    v = _lin(xs[src], p["Wv"], p["bv"]).view(E, H, C)
    ea = None
    if p.get("We") is not None:
        ea = edge_attr.double().to(dev)
        ea = ea.view(E, -1)
        e = _lin(ea, p["We"]).view(E, H, C)
        k, v = k + e, v + e
    s = (q[dst] * k).sum(-1) / math.sqrt(C)
    smax = torch.full((n, H), -math.inf, dtype=torch.float64, device=dev).scatter_reduce(
        0, dst.unsqueeze(1).expand(E, H), s, "amax", include_self=True)
    ex = (s - smax[dst]).exp()
    den = torch.zeros((n, H), dtype=torch.float64, device=dev).index_add(0, dst, ex) + 1e-16
    alpha = ex / den[dst]
    if abs_terms:
        a = alpha.detach()
        v = _lin(xs[src].abs(), p["Wv"].abs(), p["bv"].abs()).view(E, H, C)
        if ea is not None:
            v = v + _lin(ea.abs(), p["We"].abs()).view(E, H, C)
        o = torch.zeros((n, H, C), dtype=torch.float64, device=dev).index_add(0, dst, a.unsqueeze(2) * v)
        o = o.reshape(n, H * C) if concat else o.mean(1)
        if p.get("Ws") is not None:
            o = o + _lin(xd.abs(), p["Ws"].abs(), None if p["bs"] is None else p["bs"].abs())
        return o
    o = torch.zeros((n, H, C), dtype=torch.float64, device=dev).index_add(0, dst, alpha.unsqueeze(2) * v)
    o = o.reshape(n, H * C) if concat else o.mean(1)
    if p.get("Ws") is not None:
        o = o + _lin(xd, p["Ws"], p["bs"])
    if relu:
        o = torch.relu(o)
    return (o, alpha) if return_alpha else o


def dense_attention(x_src, x_dst, edge_index, p, heads, concat=True, edge_attr=None):
    """The same layer from a dense [H, n_dst, E] attention matrix built edge by edge with Python loops (the host test's
    independent check of the restatement)."""
    xs, xd = x_src.double(), (x_src if x_dst is None else x_dst).double()
    src, dst = [int(v) for v in edge_index[0]], [int(v) for v in edge_index[1]]
    n, E, H = xd.shape[0], len(src), heads
    C = p["Wq"].shape[0] // H
    out = torch.zeros((n, H, C), dtype=torch.float64)
    for i in range(n):
        es = [e for e in range(E) if dst[e] == i]
        for h in range(H):
            sl = slice(h * C, (h + 1) * C)
            q = xd[i] @ p["Wq"][sl].double().t() + p["bq"][sl].double()
            ks, vs = [], []
            for e in es:
                k = xs[src[e]] @ p["Wk"][sl].double().t() + p["bk"][sl].double()
                v = xs[src[e]] @ p["Wv"][sl].double().t() + p["bv"][sl].double()
                if p.get("We") is not None:
                    ee = edge_attr[e].double().view(-1) @ p["We"][sl].double().t()
                    k, v = k + ee, v + ee
                ks.append(float(q @ k) / math.sqrt(C))
                vs.append(v)
            if es:
                m = max(ks)
                w = [math.exp(s - m) for s in ks]
                tot = sum(w)
                out[i, h] = sum((wi / tot) * vi for wi, vi in zip(w, vs))
    o = out.reshape(n, H * C) if concat else out.mean(1)
    if p.get("Ws") is not None:
        o = o + xd @ p["Ws"].double().t() + (0 if p["bs"] is None else p["bs"].double())
    return o
