"""float64 restatement of torch_geometric.nn.GCNConv (flow source_to_target, sum aggregation) — the yardstick of the GCN
tests.  ``gcn_norm`` follows PyG's ``gcn_norm`` with ``add_remaining_self_loops``: loop edges are removed and every node gets
ONE loop whose weight is that of its (last) existing loop edge, or ``fill`` (2 when improved, else 1); deg = the weights of a
node's in-edges after that; duplicate edges count once per copy; deg 0 gives a factor 0 (PyG's inf -> 0 masking)."""
import torch


def gcn_norm(edge_index, num_nodes, edge_weight=None, improved=False, add_self_loops=True, normalize=True):
    """-> (src, dst, coef): the edges of A_hat as float64 coefficients (out[dst] += coef x[src])."""
    src = torch.as_tensor(edge_index[0]).long().cpu()
    dst = torch.as_tensor(edge_index[1]).long().cpu()
    w = torch.ones(src.shape[0], dtype=torch.float64) if edge_weight is None else torch.as_tensor(edge_weight).double().cpu()
    if not normalize:
        return src, dst, w
    if add_self_loops:
        keep = src != dst
        loop_w = torch.full((num_nodes,), 2.0 if improved else 1.0, dtype=torch.float64)
        for e in torch.nonzero(~keep).flatten().tolist():      # in edge order: the last loop edge of a node wins
            loop_w[src[e]] = w[e]
        loops = torch.arange(num_nodes)
        src, dst, w = torch.cat([src[keep], loops]), torch.cat([dst[keep], loops]), torch.cat([w[keep], loop_w])
    deg = torch.zeros(num_nodes, dtype=torch.float64).index_add_(0, dst, w)
    dinv = torch.where(deg > 0, deg.clamp(min=1e-300).pow(-0.5), torch.zeros_like(deg))
    return src, dst, dinv[src] * w * dinv[dst]


def dense_a_hat(edge_index, num_nodes, **kw):
    """A_hat as a dense float64 [num_nodes, num_nodes] matrix, rows = destinations."""
    src, dst, coef = gcn_norm(edge_index, num_nodes, **kw)
    a = torch.zeros((num_nodes, num_nodes), dtype=torch.float64)
    a.index_put_((dst, src), coef, accumulate=True)
    return a


def propagate(src, dst, coef, x, num_out=None):
    """sum_{edges} coef x[src] into the destinations (float64, any device of x)."""
    n = x.shape[0] if num_out is None else num_out
    dev = x.device
    return torch.zeros((n, x.shape[1]), dtype=x.dtype, device=dev).index_add_(
        0, dst.to(dev), coef.to(dev, x.dtype).unsqueeze(1) * x[src.to(dev)])


def gcn_forward(x, edge_index, weight, bias=None, relu=False, abs_terms=False, **kw):
    """PyG GCNConv in float64 over all of x's rows: (A_hat x) W^T + b; ``abs_terms``: the same with every factor's magnitude
    (the scale of the accuracy bar)."""
    src, dst, coef = gcn_norm(edge_index, x.shape[0], **kw)
    w = weight.double()
    if abs_terms:
        x, coef, w = x.abs(), coef.abs(), w.abs()
        bias = None if bias is None else bias.abs()
    out = propagate(src, dst, coef, x.double()) @ w.t().to(x.device)
    if bias is not None:
        out = out + bias.double().to(x.device)
    return torch.relu(out) if relu else out
