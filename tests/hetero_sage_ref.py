"""float64 restatement of ``torch_geometric.nn.HeteroConv({edge_type: SAGEConv}, aggr="sum")`` over a ``HeteroLayerGraph`` — the
yardstick of the hetero SAGE tests.  For every destination type ``dt`` and every hop's frontier entries of that type:

    out_dt[p(i)] = act( sum_{r ending in dt} [ lin_l^r( REDUCE_{j in N_r(i)} x_src(r)[j] ) + lin_r^r( x_dt[dst_rows[i]] ) ] )

``REDUCE`` = mean or sum per relation (an empty neighbourhood gives zero), ``lin_l`` carries the bias, ``lin_r`` has none and is
absent with ``root_weight=False``; ``p(i) = out_rows[i]`` (or ``i``).  EVERY relation of the module ending in ``dt`` adds its
root term and bias to every row, whether or not the hop lists edges for it."""
import torch


def params_of(layer):
    """{edge type: dict(Wl, bl, Wr, mean)} of a ``HeteroConv`` of ``SAGEConv``s, detached (float32)."""
    out = {}
    for et in layer.edge_types:
        c = layer.conv(et)
        out[et] = dict(Wl=c.lin_l.weight.detach(), bl=None if c.lin_l.bias is None else c.lin_l.bias.detach(),
                       Wr=None if c.lin_r is None else c.lin_r.weight.detach(), mean=c.aggr == "mean")
    return out


def hetero_sage_forward(xs, graph, params, relu=False, abs_terms=False):
    """``xs``: {node type: [n, F] tensor}; ``params``: ``params_of(layer)`` (its tensors may be float64 leaves that require
    grad).  ``abs_terms``: the magnitude sum of every output's terms, sum_k |c_k w_k| + |b| — the scale of the accuracy bar."""
    dev = next(iter(xs.values())).device
    f = (lambda t: t.double().abs()) if abs_terms else (lambda t: t.double())
    X = {t: f(v) for t, v in xs.items()}
    groups = {}
    for r in graph.relations:
        groups.setdefault((r.hop, r.edge_type[2]), []).append(r)
    out = {}
    for (hop, dt), mine in sorted(groups.items()):
        n_f = mine[0].n_rows
        if n_f == 0:
            continue
        listed = {r.edge_type: r for r in mine}
        N = next(p["Wl"].shape[0] for et, p in params.items() if et[2] == dt)
        y = torch.zeros((n_f, N), dtype=torch.float64, device=dev)
        for et, p in sorted(params.items()):
            if et[2] != dt:
                continue
            r = listed.get(et)
            agg = torch.zeros((n_f, X[et[0]].shape[1]), dtype=torch.float64, device=dev)
            if r is not None and r.n_edges > 0:
                deg = (r.row_ptr[1:] - r.row_ptr[:-1]).long()
                row = torch.repeat_interleave(torch.arange(n_f, device=dev), deg)
                agg = agg.index_add(0, row, X[et[0]][r.col.long()[:r.n_edges]])
                if p["mean"]:
                    agg = agg / deg.clamp(min=1).unsqueeze(1)
            y = y + agg @ f(p["Wl"]).t()          # (an empty neighbourhood: zero — the weight still gets a (zero) gradient)
            if p["bl"] is not None:
                y = y + f(p["bl"])
            if p["Wr"] is not None:
                y = y + X[dt][mine[0].dst_rows] @ f(p["Wr"]).t()
        if relu and not abs_terms:
            y = torch.relu(y)
        rows = mine[0].out_rows
        if dt not in out:
            out[dt] = torch.zeros((graph.n_out[dt], N), dtype=torch.float64, device=dev)
        if rows is None:
            out[dt] = y
        else:
            out[dt] = out[dt].index_copy(0, rows, y)
    return out
