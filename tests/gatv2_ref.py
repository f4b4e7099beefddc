"""float64 restatement of torch_geometric.nn.GATv2Conv (flow source_to_target, no dropout, no edge features) — the yardstick of
the GATv2Conv tests.  For edge j -> i and head h: XL = lin_l(x_src), XR = lin_r(x_dst),
e_ijh = sum_c att[h, c] LeakyReLU(XL[j, h, c] + XR[i, h, c]), alpha = softmax over the edges into i, out_i = sum_j alpha_ijh
XL[j, h, :], heads concatenated or averaged, plus bias.  A destination without edges gets the bias alone.  Every edge of
``edge_index`` is an ordinary edge — loops and duplicates too; self loops are whatever edges the caller lists for them."""
import math

import torch


def _lin(x, w, b=None):
    y = x @ w.double().t()
    return y if b is None else y + b.double()


def params_of(conv):
    """The parameters of a GATv2Conv (or anything with PyG's names) as a dict of detached tensors."""
    d = lambda t: None if t is None else t.detach()   # noqa: E731
    return dict(Wl=d(conv.lin_l.weight), bl=d(conv.lin_l.bias), Wr=d(conv.lin_r.weight), br=d(conv.lin_r.bias), att=d(conv.att),
                bias=d(conv.bias))


def gatv2_forward(x_src, x_dst, edge_index, p, heads, concat=True, negative_slope=0.2, relu=False, abs_terms=False,
                  return_alpha=False):
    """PyG GATv2Conv in float64 over x_dst's rows (``x_dst`` None: x_src's).  ``p``: ``params_of(conv)`` (tensors may require
    grad).  ``abs_terms``: the magnitude sum of the output's terms — sum_j alpha_ij (|x| |W_l|^T + |b_l|)[j] per head (alpha the
    true weights, averaged like the output) + |bias| — the scale of the accuracy bar."""
    dev = x_src.device
    xs = x_src.double()
    xd = xs if x_dst is None else x_dst.double()
    src = torch.as_tensor(edge_index[0]).long().to(dev)
    dst = torch.as_tensor(edge_index[1]).long().to(dev)
    n, E, H = xd.shape[0], src.shape[0], heads
    C = p["Wl"].shape[0] // H
    xl = _lin(xs, p["Wl"], p["bl"]).view(-1, H, C)
    xr = _lin(xd, p["Wr"], p["br"]).view(n, H, C)
    s = torch.nn.functional.leaky_relu(xl[src] + xr[dst], negative_slope)
    e = (s * p["att"].double().view(1, H, C)).sum(-1)
    emax = torch.full((n, H), -math.inf, dtype=torch.float64, device=dev).scatter_reduce(
        0, dst.unsqueeze(1).expand(E, H), e, "amax", include_self=True)
    ex = (e - emax[dst]).exp()
    den = torch.zeros((n, H), dtype=torch.float64, device=dev).index_add(0, dst, ex)
    alpha = ex / den[dst]
    bias = p.get("bias")
    if abs_terms:
        v = _lin(xs.abs(), p["Wl"].abs(), None if p["bl"] is None else p["bl"].abs()).view(-1, H, C)[src]
        o = torch.zeros((n, H, C), dtype=torch.float64, device=dev).index_add(0, dst, alpha.detach().unsqueeze(2) * v)
        o = o.reshape(n, H * C) if concat else o.mean(1)
        return o if bias is None else o + bias.double().abs()
    o = torch.zeros((n, H, C), dtype=torch.float64, device=dev).index_add(0, dst, alpha.unsqueeze(2) * xl[src])
    o = o.reshape(n, H * C) if concat else o.mean(1)
    if bias is not None:
        o = o + bias.double()
    if relu:
        o = torch.relu(o)
    return (o, alpha) if return_alpha else o


def gatv2_by_hand(x_src, x_dst, edge_index, p, heads, concat=True, negative_slope=0.2):
    """The same layer edge by edge with Python loops and ``math.exp`` (the host test's independent check of the restatement)."""
    xs, xd = x_src.double(), (x_src if x_dst is None else x_dst).double()
    src, dst = [int(v) for v in edge_index[0]], [int(v) for v in edge_index[1]]
    n, E, H = xd.shape[0], len(src), heads
    C = p["Wl"].shape[0] // H
    att = p["att"].double().view(H, C)
    out = torch.zeros((n, H, C), dtype=torch.float64)
    for i in range(n):
        es = [e for e in range(E) if dst[e] == i]
        for h in range(H):
            sl = slice(h * C, (h + 1) * C)
            r = xd[i] @ p["Wr"][sl].double().t() + (0 if p["br"] is None else p["br"][sl].double())
            logits, rows = [], []
            for e in es:
                left = xs[src[e]] @ p["Wl"][sl].double().t() + (0 if p["bl"] is None else p["bl"][sl].double())
                z = left + r
                logits.append(sum(float(att[h, c]) * (float(z[c]) if float(z[c]) > 0 else negative_slope * float(z[c]))
                                  for c in range(C)))
                rows.append(left)
            if es:
                m = max(logits)
                w = [math.exp(s - m) for s in logits]
                tot = sum(w)
                out[i, h] = sum((wi / tot) * vi for wi, vi in zip(w, rows))
    o = out.reshape(n, H * C) if concat else out.mean(1)
    return o if p.get("bias") is None else o + p["bias"].double()
