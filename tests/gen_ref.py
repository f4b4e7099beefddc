"""float64 restatement of torch_geometric.nn.GENConv (aggr="softmax", flow source_to_target) in plain index ops — the yardstick of
the GENConv tests: xs = lin_src(x), xd = lin_dst(x_dst), m_j = relu(xs_j) + eps, agg_i[c] = sum_j p_jc m_jc with
p_jc = exp(t m_jc - max) / sum_k exp(t m_kc - max) over the edges into i (an explicit per-channel maximum; 0 without edges),
out = mlp(agg + xd); every edge of ``edge_index`` is an ordinary edge, loops and duplicates too.  The parameters go by the layer's own
state-dict names (``lin_src.weight``, ``mlp.0.weight``, ...; a 1-d ``mlp.{i}.weight`` is a BatchNorm1d in training mode: batch
statistics, biased variance, eps 1e-5); a ReLU sits in front of every Linear of the mlp but the first."""
import torch


def params_of(conv):
    return {k: v.detach() for k, v in conv.named_parameters() if k != "aggr_module.t"}


def gen_forward(x, x_dst, edge_index, p, t, eps=1e-7, relu=False):
    """``(out, scale)`` over ``x_dst``'s rows (destination i of ``edge_index`` is row i of ``x_dst``; ``x_dst`` None: no root term).
    ``p``: ``params_of`` (tensors may require grad), ``t`` a float64 tensor.  ``scale``: the magnitude sum of the output's terms — the
    same chain over the absolute values of every input, weight and bias with the softmax weights as they are (a batch norm:
    (|z| + mean |z|) |gamma| / std + |beta|, the statistics as they are)."""
    mag = lambda v: v.detach().abs()      # noqa: E731

    def lin(y, s, name):
        if name + ".weight" in p:
            y, s = y @ p[name + ".weight"].t(), s @ mag(p[name + ".weight"]).t()
            if name + ".bias" in p:
                y, s = y + p[name + ".bias"], s + mag(p[name + ".bias"])
        return y, s
    src, dst = edge_index[0].long(), edge_index[1].long()
    xs, sxs = lin(x, mag(x), "lin_src")
    n, C = int(dst.max()) + 1 if x_dst is None else x_dst.shape[0], xs.shape[1]
    zeros = torch.zeros((n, C), dtype=torch.float64, device=x.device)
    m, sm = torch.relu(xs[src]) + eps, sxs[src] + eps
    z = t * m
    top = torch.full_like(zeros, -float("inf")).scatter_reduce(0, dst.unsqueeze(1).expand_as(z), z.detach(), "amax")
    w = torch.exp(z - top[dst])
    pw = w / zeros.index_add(0, dst, w)[dst]
    y, s = zeros.index_add(0, dst, pw * m), zeros.index_add(0, dst, pw.detach() * sm)
    if x_dst is not None:
        xd, sxd = lin(x_dst, mag(x_dst), "lin_dst")
        y, s = y + xd, s + sxd
    for i in sorted({int(k.split(".")[1]) for k in p if k.startswith("mlp.")}):
        name = "mlp.%d" % i
        if p[name + ".weight"].dim() == 2:
            y, s = lin(torch.relu(y) if i > 0 else y, s, name)
        else:
            mean, std = y.mean(0), torch.sqrt(y.var(0, unbiased=False) + 1e-5)
            y = (y - mean) / std * p[name + ".weight"] + p[name + ".bias"]
            s = (s + s.mean(0)) / std.detach() * mag(p[name + ".weight"]) + mag(p[name + ".bias"])
    return (torch.relu(y) if relu else y), s
