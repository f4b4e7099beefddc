"""float64 restatement of torch_geometric.nn.GATv2Conv(edge_dim=D) (flow source_to_target, no dropout) — the yardstick of the
GATv2EdgeConv tests: tests/gatv2_ref.py with ``lin_edge`` of every edge's row inside the LeakyReLU,
e_ijh = sum_c att[h, c] LeakyReLU(XL[j] + XR[i] + W_e a_ij)[h, c]; the message stays XL[j].  Every edge of ``edge_index`` is an
ordinary edge with its row of ``edge_rows``; self loops are whatever edges — and fill rows — the caller lists for them."""
import math

import torch

from gatv2_ref import _lin, params_of


def edge_params_of(conv):
    return dict(params_of(conv), We=conv.lin_edge.weight.detach())


def with_loops(edge_index, edge_rows, loop_rows, fill):
    """The edge list and rows with one loop ``loop_rows[i] -> loop_rows[i]`` per destination in front, its row: ``fill`` (a float),
    or — "mean" — the mean of the rows of the destination's edges (zeros without any)."""
    n, dst = loop_rows.shape[0], edge_index[1]
    rows = edge_rows.double()
    if fill == "mean":
        where = torch.full((int(max(int(loop_rows.max()), int(dst.max()) if dst.numel() else 0)) + 1,), -1, device=dst.device)
        where[loop_rows] = torch.arange(n, device=dst.device)
        at = where[dst]
        cnt = torch.zeros(n, dtype=torch.float64, device=dst.device).index_add(0, at, torch.ones_like(rows[:, 0]))
        f = torch.zeros((n, rows.shape[1]), dtype=torch.float64, device=dst.device).index_add(0, at, rows) / cnt.clamp(min=1).unsqueeze(1)
    else:
        f = torch.full((n, rows.shape[1]), float(fill), dtype=torch.float64, device=dst.device)
    return torch.cat([torch.stack([loop_rows, loop_rows]), edge_index], 1), torch.cat([f, rows])


def gatv2_edge_forward(x, edge_index, edge_rows, p, heads, concat=True, negative_slope=0.2, relu=False, abs_terms=False,
                       return_alpha=False):
    """Over x's rows; ``p``: ``edge_params_of(conv)`` (tensors may require grad).  ``abs_terms``: the magnitude sum of the output's
    terms, as ``gatv2_ref.gatv2_forward`` defines it (the message has the same terms)."""
    dev, xs, H = x.device, x.double(), heads
    src, dst = edge_index[0].long().to(dev), edge_index[1].long().to(dev)
    n, E, C = xs.shape[0], src.shape[0], p["Wl"].shape[0] // H
    xl = _lin(xs, p["Wl"], p["bl"]).view(-1, H, C)
    xr = _lin(xs, p["Wr"], p["br"]).view(n, H, C)
    s = xl[src] + xr[dst] + _lin(edge_rows.double(), p["We"]).view(E, H, C)
    e = (torch.nn.functional.leaky_relu(s, negative_slope) * p["att"].double().view(1, H, C)).sum(-1)
    emax = torch.full((n, H), -math.inf, dtype=torch.float64, device=dev).scatter_reduce(
        0, dst.unsqueeze(1).expand(E, H), e, "amax", include_self=True)
    ex = (e - emax[dst]).exp()
    alpha = ex / torch.zeros((n, H), dtype=torch.float64, device=dev).index_add(0, dst, ex)[dst]
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
