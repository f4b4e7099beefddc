"""float64 restatement of torch_geometric.nn.PNAConv (flow source_to_target, no edge features) in plain index ops — the yardstick of
the PNAConv tests.  Per tower t: m_e = pre_nns[t]([x_i | x_j]) for every edge e = (j -> i); per channel the aggregators sum, mean,
min, max, var = mean(m^2) - mean(m)^2 and std = sqrt(relu(var) + 1e-5), min and max taken at the LOWEST slot (position in
``edge_index``) among the row's edges that hold the extreme, every statistic 0 for a row without edges; the scalers of the in-degree
clamped to >= 1; out = lin(cat_t post_nns[t]([x_i | scaler-major concat])).  The parameters go by the layer's own state-dict names;
a ReLU sits between the Linears of a pre / post network."""
import torch


def params_of(conv):
    return {k: v.detach() for k, v in conv.named_parameters()}


def pna_forward(x, x_dst, edge_index, p, aggregators, scalers, avg_lin, avg_log, towers=1, divide_input=False, relu=False):
    """``(out, scale)`` over ``x_dst``'s rows (destination i of ``edge_index`` is row i of ``x_dst``).  ``scale``: the magnitude sum of
    the output's terms — the same chain over the absolute values of every input, weight and bias (var: mean(|m|^2) + mean(|m|)^2,
    std: its root with the 1e-5; min / max: the magnitude at the chosen slot)."""
    mag = lambda v: v.detach().abs()      # noqa: E731
    src, dst = edge_index[0].long(), edge_index[1].long()
    n, E, T = x_dst.shape[0], src.shape[0], towers
    split = lambda v: v.view(v.shape[0], T, -1) if divide_input else v.unsqueeze(1).expand(-1, T, -1)      # noqa: E731

    def net(name, y, s):
        for k in sorted({int(key.split(".")[2]) for key in p if key.startswith(name + ".")}):
            w, b = p["%s.%d.weight" % (name, k)], p["%s.%d.bias" % (name, k)]
            y, s = (torch.relu(y) if k > 0 else y) @ w.t() + b, s @ mag(w).t() + mag(b)
        return y, s
    deg = torch.bincount(dst, minlength=n)
    has, d = (deg > 0).unsqueeze(1), deg.clamp(min=1).double().unsqueeze(1)
    lg = torch.log(d + 1)
    scaler = {"identity": torch.ones_like(d), "amplification": lg / avg_log, "attenuation": avg_log / lg, "linear": d / avg_lin,
              "inverse_linear": avg_lin / d}
    outs, souts = [], []
    for t in range(T):
        xi, xj = split(x_dst)[:, t], split(x)[:, t]
        m, sm = net("pre_nns.%d" % t, torch.cat([xi[dst], xj[src]], 1), torch.cat([mag(xi)[dst], mag(xj)[src]], 1))
        zeros = torch.zeros((n, m.shape[1]), dtype=torch.float64, device=x.device)
        add = lambda v: zeros.index_add(0, dst, v)      # noqa: E731
        mean, smean = add(m) / d, add(sm) / d
        var, svar = add(m * m) / d - mean * mean, add(sm * sm) / d + smean * smean
        idx, slot = dst.unsqueeze(1).expand_as(m), torch.arange(E, device=x.device).unsqueeze(1).expand_as(m)

        def extreme(kind):
            ext = zeros.scatter_reduce(0, idx, m.detach(), kind, include_self=False)
            first = torch.full_like(zeros, E, dtype=torch.int64).scatter_reduce(0, idx, torch.where(m.detach() == ext[dst], slot, E), "amin")
            first = first.clamp(max=E - 1)
            return torch.where(has, m.gather(0, first), zeros), torch.where(has, sm.gather(0, first), zeros)
        stat = {"sum": lambda: (mean * d, smean * d), "mean": lambda: (mean, smean), "min": lambda: extreme("amin"),
                "max": lambda: extreme("amax"), "var": lambda: (var, svar),
                "std": lambda: (torch.where(has, torch.sqrt(torch.relu(var) + 1e-5), zeros), torch.where(has, torch.sqrt(svar + 1e-5), zeros))}
        stats = [stat[k]() for k in aggregators]
        cat = torch.cat([xi] + [v * scaler[k] for k in scalers for v, _ in stats], 1)
        scat = torch.cat([mag(xi)] + [s * scaler[k] for k in scalers for _, s in stats], 1)
        o, so = net("post_nns.%d" % t, cat, scat)
        outs.append(o)
        souts.append(so)
    y = torch.cat(outs, 1) @ p["lin.weight"].t() + p["lin.bias"]
    s = torch.cat(souts, 1) @ mag(p["lin.weight"]).t() + mag(p["lin.bias"])
    return (torch.relu(y) if relu else y), s
