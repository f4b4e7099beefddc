"""float64 restatement of torch_geometric.nn.GINEConv (flow source_to_target) in plain index ops — the yardstick of the GINEConv
tests: out_i = nn((1 + eps) x_dst_i + sum_{e = (j -> i)} ReLU(x_j + lin(edge_rows_e))), every edge of ``edge_index`` an ordinary
edge (loops and duplicates too).  ``nn`` is given as its Linear layers with a ReLU between them, an optional ReLU behind."""
import torch


def params_of(conv, lins):
    """The layer's tensors by the restatement's names: ``lins`` = the Linear modules of ``conv.nn`` in order."""
    p = {"eps": conv.eps.detach()}
    if conv.lin is not None:
        p.update(We=conv.lin.weight.detach(), be=conv.lin.bias.detach())
    for k, lin in enumerate(lins, 1):
        p.update({"W%d" % k: lin.weight.detach(), "b%d" % k: lin.bias.detach()})
    return p


def gine_forward(x, x_dst, edge_index, edge_rows, p, relu=False, abs_terms=False):
    """Over ``x_dst``'s rows (destination i of ``edge_index`` is row i of ``x_dst``).  ``p``: ``params_of`` (tensors may require
    grad); without ``We`` the edge rows are as wide as x.  ``abs_terms``: the magnitude sum of the output's terms — the same
    formula over the absolute values of every input, weight and bias."""
    f = (lambda t: t.double().abs()) if abs_terms else (lambda t: t.double())
    src, dst = edge_index[0].long(), edge_index[1].long()
    e = f(edge_rows)
    if "We" in p:
        e = e @ f(p["We"]).t() + f(p["be"])
    msg = f(x)[src] + e
    msg = msg if abs_terms else torch.relu(msg)
    y = torch.zeros((x_dst.shape[0], x.shape[1]), dtype=torch.float64, device=x.device).index_add(0, dst, msg)
    y = y + (1.0 + f(p["eps"])) * f(x_dst)
    k = 1
    while "W%d" % k in p:
        y = y @ f(p["W%d" % k]).t() + f(p["b%d" % k])
        if "W%d" % (k + 1) in p or relu:
            y = y if abs_terms else torch.relu(y)
        k += 1
    return y
