"""float64 restatement of torch_geometric.nn.GINConv (flow source_to_target, sum aggregation) — the yardstick of the GIN
tests: ``agg = index_add_ over the edges of x[src]  +  (1 + eps) x_dst`` (every edge counts: loop edges and duplicates once per
copy), then the MLP ``relu(agg W1^T + b1) W2^T + b2`` (``W2 = None``: the first product alone, ReLU on request)."""
import torch


def gin_aggregate(x, edge_index, eps=0.0, x_dst=None, num_dst=None, root=True, abs_terms=False):
    """-> agg float64 [num_dst, F]; ``x_dst`` None: the destinations are x's own rows; ``root=False``: no ``(1 + eps) x_dst``
    term (PyG's ``(x_src, None)``); ``abs_terms``: the magnitude sum of the same terms."""
    x = x.double()
    src, dst = edge_index[0].long().to(x.device), edge_index[1].long().to(x.device)
    xd = x if x_dst is None else x_dst.double()
    n = (xd.shape[0] if root else int(dst.max()) + 1) if num_dst is None else num_dst
    c = 1.0 + float(eps)
    if abs_terms:
        x, xd, c = x.abs(), xd.abs(), abs(c)
    agg = torch.zeros((n, x.shape[1]), dtype=torch.float64, device=x.device).index_add_(0, dst, x[src])
    return agg + c * xd[:n] if root else agg


def mlp(agg, w1, b1=None, w2=None, b2=None, relu_hidden=True, relu=False, abs_terms=False):
    """The chain behind the aggregate in float64; ``abs_terms``: ``agg @ |W1|^T + |b1|``, then ``@ |W2|^T + |b2|`` (agg being
    the magnitude sum already) — the scale of the accuracy bar, no activation."""
    f = (lambda t: None if t is None else t.double().abs().to(agg.device)) if abs_terms else (
        lambda t: None if t is None else t.double().to(agg.device))
    w1, b1, w2, b2 = f(w1), f(b1), f(w2), f(b2)
    h = agg @ w1.t()
    if b1 is not None:
        h = h + b1
    if w2 is None:
        return torch.relu(h) if (relu_hidden or relu) and not abs_terms else h
    if relu_hidden and not abs_terms:
        h = torch.relu(h)
    out = h @ w2.t()
    if b2 is not None:
        out = out + b2
    return torch.relu(out) if relu and not abs_terms else out


def gin_forward(x, edge_index, w1, b1=None, w2=None, b2=None, eps=0.0, x_dst=None, num_dst=None, root=True, relu_hidden=True,
                relu=False, abs_terms=False):
    """PyG GINConv with the GIN paper's MLP in float64 (``abs_terms``: the magnitude sum pushed through the chain)."""
    agg = gin_aggregate(x, edge_index, eps, x_dst, num_dst, root, abs_terms)
    return mlp(agg, w1, b1, w2, b2, relu_hidden, relu, abs_terms)
