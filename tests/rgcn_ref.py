"""float64 restatement of torch_geometric.nn.RGCNConv / FastRGCNConv (flow source_to_target) — the yardstick of the RGCN
tests.  PyG's relation-by-relation loop: for every relation r, the edges of type r are propagated on their own, averaged per
destination over that relation's edges alone (aggr "mean"; "add" / "sum": summed), and multiplied by W_r = sum_b comp[r, b]
basis_b (or weight[r] without bases); x @ root and bias are added once.  A sampled loop edge is an ordinary edge, duplicate
edges count once per copy, a relation with no edge into a node contributes 0."""
import torch


def relation_weights(weight, comp=None):
    """W_r [R, F, N] (float64) from the layer's parameters."""
    w = weight.double()
    if comp is None:
        return w
    B, F, N = w.shape
    return (comp.double() @ w.reshape(B, F * N)).view(comp.shape[0], F, N)


def rgcn_forward(x, edge_index, edge_type, weight, comp=None, root=None, bias=None, aggr="mean", relu=False, abs_terms=False,
                 num_relations=None):
    """PyG RGCNConv in float64 over all of x's rows.  ``abs_terms``: the same with every factor's magnitude —
    sum |n| |comp| |basis| |x| + |x_self| |root| + |bias| — the scale of the accuracy bar."""
    dev = x.device
    x = x.double()
    src = torch.as_tensor(edge_index[0]).long().to(dev)
    dst = torch.as_tensor(edge_index[1]).long().to(dev)
    et = torch.as_tensor(edge_type).long().to(dev)
    if abs_terms:
        x, weight = x.abs(), weight.abs()
        comp = None if comp is None else comp.abs()
        root = None if root is None else root.abs()
        bias = None if bias is None else bias.abs()
    W = relation_weights(weight, comp).to(dev)
    R = W.shape[0] if num_relations is None else num_relations
    n, N = x.shape[0], W.shape[2]
    out = torch.zeros((n, N), dtype=torch.float64, device=dev)
    for r in torch.unique(et).tolist():
        assert 0 <= r < R
        m = et == r
        s, d = src[m], dst[m]
        h = torch.zeros((n, x.shape[1]), dtype=torch.float64, device=dev).index_add_(0, d, x[s])
        if aggr == "mean":
            cnt = torch.bincount(d, minlength=n).clamp(min=1).double()
            h = h / cnt.unsqueeze(1)
        out = out + h @ W[r]
    if root is not None:
        out = out + x @ root.double().to(dev)
    if bias is not None:
        out = out + bias.double().to(dev)
    return torch.relu(out) if relu else out


def dense_relation_adjacency(edge_index, edge_type, num_nodes, num_relations, aggr="mean"):
    """A [R, n, n] float64 (rows = destinations): entry (r, i, j) = the weight of x_j in relation r's aggregate for i."""
    src, dst = torch.as_tensor(edge_index[0]).long(), torch.as_tensor(edge_index[1]).long()
    et = torch.as_tensor(edge_type).long()
    a = torch.zeros((num_relations, num_nodes, num_nodes), dtype=torch.float64)
    a.index_put_((et, dst, src), torch.ones(src.shape[0], dtype=torch.float64), accumulate=True)
    if aggr == "mean":
        a = a / a.sum(2, keepdim=True).clamp(min=1)
    return a
