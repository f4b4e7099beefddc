"""float64 restatement of ``torch_geometric.nn.HeteroConv({edge_type: TransformerConv}, aggr="sum")`` over a ``HeteroLayerGraph``
— the yardstick of the hetero transformer tests.  For every destination type ``dt`` and every hop's frontier entries of it:

    out_dt[p(i)] = act( sum_{r ending in dt} TransformerConv_r( (x_src(r), x_dt[dst_rows]) , edges of r in the hop )[i] )

through ``transformer_ref.transformer_forward`` per relation hop (its softmax is per relation; a row without edges in a relation
gets that relation's skip term alone), ReLU after the sum, ``p(i) = out_rows[i]`` (or ``i``).  EVERY relation of the module
ending in ``dt`` whose source type has input rows adds its skip term to every row, whether or not the hop lists edges for it.
``edge_attr_dict[et]`` is hop-major per edge type; a relation hop reads rows ``[edge_base, edge_base + n_edges)``."""
import torch

import transformer_ref as tref


def params_of(layer):
    """{edge type: dict(p=transformer_ref.params_of(conv), heads, concat)} of a ``HeteroConv`` of ``TransformerConv``s."""
    return {et: dict(p=tref.params_of(layer.conv(et)), heads=layer.conv(et).heads, concat=layer.conv(et).concat)
            for et in layer.edge_types}


def relation_coo(r):
    """(source row, destination row) int64 of every edge of a ``RelationHop``, in CSR order."""
    n, dev = r.n_rows, r.row_ptr.device
    deg = (r.row_ptr[1:] - r.row_ptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n, device=dev), deg)
    return torch.stack([r.col.long()[:r.n_edges], dst])


def hetero_transformer_forward(xs, graph, params, edge_attr_dict=None, relu=False, abs_terms=False):
    """``xs``: {node type: [n, F] tensor}; ``params``: ``params_of(layer)`` (the tensors of its ``p`` may be float64 leaves that
    require grad).  ``abs_terms``: the magnitude sum of every output's terms (``transformer_forward(abs_terms=True)`` summed
    over the relations) — the scale of the accuracy bar."""
    dev = next(iter(xs.values())).device
    groups = {}
    for r in graph.relations:
        groups.setdefault((r.hop, r.edge_type[2]), []).append(r)
    out = {}
    for (hop, dt), mine in sorted(groups.items()):
        n_f = mine[0].n_rows
        if n_f == 0:
            continue
        listed = {r.edge_type: r for r in mine}
        xd = xs[dt][mine[0].dst_rows]
        y = None
        for et, q in sorted(params.items()):
            if et[2] != dt or et[0] not in xs:
                continue
            r = listed.get(et)
            p, ea = q["p"], None
            if r is not None and r.n_edges > 0:
                coo = relation_coo(r)
                if p.get("We") is not None:
                    ea = edge_attr_dict[et][r.edge_base:r.edge_base + r.n_edges]
            else:       # no edge of the relation in this hop: the skip term alone (no edge, so lin_edge has nothing to read)
                coo, p = torch.zeros((2, 0), dtype=torch.int64, device=dev), dict(p, We=None)
            o = tref.transformer_forward(xs[et[0]], xd, coo, p, q["heads"], concat=q["concat"], edge_attr=ea,
                                         abs_terms=abs_terms)
            y = o if y is None else y + o
        if relu and not abs_terms:
            y = torch.relu(y)
        rows = mine[0].out_rows
        if dt not in out:
            out[dt] = torch.zeros((graph.n_out[dt], y.shape[1]), dtype=torch.float64, device=dev)
        if rows is None:
            out[dt] = y
        else:
            out[dt] = out[dt].index_copy(0, rows, y)
    return out
