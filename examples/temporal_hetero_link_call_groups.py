#!/usr/bin/env python
"""Temporal heterogeneous link prediction over call groups — the training loop of the reference's
python/cugraph-pyg/cugraph_pyg/examples/movielens_mnmg.py on a planted user - item graph: typed seed edges `user -> item` with
`edge_label_time = time - 1` and `time_attr="time"` (a seed edge only sees ratings made before it), binary negatives x 2, the
same fan-out on `rates` and `rev_rates`, a heterogeneous GraphSAGE encoder with one layer per hop, the two-`Linear`
`EdgeDecoder`, BCE.

  * `LinkNeighborLoader(..., edge_label_time=, time_attr=).hetero_call_groups()` -> `HeteroLinkCallGroup`: the negatives of G
    mini-batches, one row-wise de-duplication per endpoint type, the seed time of every unique endpoint (the time of the first
    pair that names it: `graph_ops.rows_first_values`) and ONE temporal walk (`HeteroPygWalk(temporal_comparison=)`: every (hop,
    edge type) on `wgamd_sample_hop_pyg_temporal_nosync`, a reach-time list per node type) — nothing read back but the sizes;
  * `wholegraph_amd.nn.HeteroConv({edge_type: SAGEConv})` per hop over `grp.layer_graph(j)`, `x_dict` a dict of `LazyRows`;
  * `wholegraph_amd.nn.EdgeDecoder.loss` over `(h["user"], h["item"], grp.edge_label_index)`; one optimizer step per call group.

`--per-batch` is the loop this replaces: `for batch in loader` (the one-batch-at-a-time temporal route), the same parameters
applied with torch ops to every mini-batch's `HeteroData`, one optimizer step per mini-batch.

    python examples/temporal_hetero_link_call_groups.py [--users 20000] [--items 4000] [--fanout 5 5] [--epochs 3] [--per-batch]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cugraph-gnn_amd")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from cugraph_pyg_amd.data import FeatureStore, GraphStore  # noqa: E402
from cugraph_pyg_amd.loader import LinkNeighborLoader  # noqa: E402
from wholegraph_amd import nn as wnn  # noqa: E402

F_USER, F_ITEM = 32, 48
RATES, REV_RATES = ("user", "rates", "item"), ("item", "rev_rates", "user")
LAST_EPOCH = {}       # what the last epoch of the last `main` call measured


def planted_ratings(U, I, E, C, horizon, dev, g):
    """`rates` edges user -> item, 90 % of them inside the user's community, each with an int64 time in [0, horizon); the
    features are noisy one-hots of the community, of a different width per type."""
    cu, ci = torch.arange(U, device=dev) % C, torch.arange(I, device=dev) % C
    user = torch.randint(0, U, (E,), generator=g, device=dev)
    inside = torch.rand(E, generator=g, device=dev) < 0.9
    peer = (torch.randint(0, max(I // C, 1), (E,), generator=g, device=dev) * C + cu[user]).clamp_(max=I - 1)
    item = torch.where(inside, peer, torch.randint(0, I, (E,), generator=g, device=dev))
    when = torch.randint(0, horizon, (E,), generator=g, device=dev)
    xu = 0.5 * torch.randn((U, F_USER), generator=g, device=dev)
    xu[torch.arange(U, device=dev), cu % F_USER] += 1.0
    xi = 0.5 * torch.randn((I, F_ITEM), generator=g, device=dev)
    xi[torch.arange(I, device=dev), ci % F_ITEM] += 1.0
    return torch.stack([user, item]), when, xu, xi


def plain_forward(layers, data):
    """The encoder on ONE mini-batch's `HeteroData` in torch ops: per edge type lin_l(mean over a node's in-edges) + lin_r(the
    node's own row), summed over the edge types that end in the node's type, ReLU between the layers."""
    h = {t: data[t].x for t in ("user", "item")}
    for j, layer in enumerate(layers):
        out = {}
        for et in layer.edge_types:
            conv, (src, dst) = layer.conv(et), data[et].edge_index
            xs, xd = h[et[0]], h[et[2]]
            deg = torch.zeros(xd.shape[0], device=xd.device).index_add_(0, dst, torch.ones(dst.shape[0], device=xd.device))
            agg = torch.zeros((xd.shape[0], xs.shape[1]), device=xd.device).index_add_(0, dst, xs[src]) / deg.clamp(min=1).unsqueeze(1)
            y = conv.lin_l(agg) + conv.lin_r(xd)
            out[et[2]] = y if et[2] not in out else out[et[2]] + y
        h = {t: v.relu() for t, v in out.items()} if j + 1 < len(layers) else out
    return h


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=20_000)
    ap.add_argument("--items", type=int, default=4_000)
    ap.add_argument("--avg-degree", type=int, default=25, help="`rates` edges per user")
    ap.add_argument("--communities", type=int, default=20)
    ap.add_argument("--horizon", type=int, default=1000, help="edge times are uniform in [0, horizon)")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--group", type=int, default=8, help="mini-batches per call group (= per optimizer step)")
    ap.add_argument("--fanout", type=int, nargs="+", default=[5, 5], help="per hop, on both edge types; one layer per hop (2 or 3)")
    ap.add_argument("--train-edges", type=int, default=0, help="seed edges per epoch (0: a quarter of the ratings)")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--per-batch", action="store_true", help="`for batch in loader` with torch ops: the loop the call groups replace")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs an MI355X (there is no CPU fallback)"
    assert 2 <= len(args.fanout) <= 3
    dev = torch.device("cuda")
    torch.manual_seed(0)
    g = torch.Generator(device=dev).manual_seed(0)
    U, I, E = args.users, args.items, args.users * args.avg_degree
    rates, when, xu, xi = planted_ratings(U, I, E, args.communities, args.horizon, dev, g)
    graph_store, feature_store = GraphStore(), FeatureStore()
    graph_store[RATES, "coo", False, (U, I)] = rates
    graph_store[REV_RATES, "coo", False, (I, U)] = rates.flip(0)
    feature_store["user", "x", None] = xu
    feature_store["item", "x", None] = xi
    feature_store[RATES, "time", None] = when
    feature_store[REV_RATES, "time", None] = when
    train = torch.randperm(E, generator=g, device=dev)[: args.train_edges or E // 4]
    fan = {et: list(args.fanout) for et in (RATES, REV_RATES)}
    # a mini-batch of B seed edges and 2 B negatives seeds 3 B endpoints of either type
    loader = LinkNeighborLoader((feature_store, graph_store), num_neighbors=fan, edge_label_index=(RATES, rates[:, train]),
                                edge_label_time=when[train] - 1, time_attr="time", batch_size=args.batch_size,
                                neg_sampling=("binary", 2.0), shuffle=True, local_seeds_per_call=args.group * 6 * args.batch_size)
    width = {"user": F_USER, "item": F_ITEM}
    layers = torch.nn.ModuleList(
        [wnn.HeteroConv({et: wnn.SAGEConv((width[et[0]], width[et[2]]) if j == 0 else (args.hidden, args.hidden), args.hidden)
                         for et in fan}) for j in range(len(args.fanout))]).to(dev)
    decoder = wnn.EdgeDecoder(args.hidden).to(dev)
    opt = torch.optim.Adam(list(layers.parameters()) + list(decoder.parameters()), lr=0.01)

    def group_step(grp):
        h = grp.x_dict                                      # LazyRows: nothing gathered
        for j, layer in enumerate(layers):
            h = layer(h, grp.layer_graph(j), act="relu" if j + 1 < len(layers) else None)
        hu, hi = h["user"], h["item"]                       # rows = the unique endpoints of all mini-batches, per type
        eli, label = grp.edge_label_index, (grp.edge_label > 0).float()
        loss = decoder.loss(hu, hi, eli, label)
        with torch.no_grad():
            score = decoder(hu.detach(), hi.detach(), eli)
        return loss, score, label, grp.num_edges

    def batch_step(batch):
        h = plain_forward(layers, batch)
        st = batch[RATES]
        eli, label = st.edge_label_index, (st.edge_label > 0).float()
        score = decoder.lin2(decoder.lin1(torch.cat([h["user"][eli[0]], h["item"][eli[1]]], dim=-1)).relu()).view(-1)
        return F.binary_cross_entropy_with_logits(score, label), score.detach(), label, sum(
            int(batch[et].edge_index.shape[1]) for et in fan)

    loss_avg = acc = 0.0
    for epoch in range(args.epochs):
        torch.cuda.synchronize()
        t0, edges, pairs = time.perf_counter(), 0, 0
        total = torch.zeros((), device=dev)                 # (device-side running sums: no read-back per step)
        correct = torch.zeros((), device=dev)
        for unit in (loader if args.per_batch else loader.hetero_call_groups()):
            loss, score, label, n_edges = (batch_step if args.per_batch else group_step)(unit)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            with torch.no_grad():
                correct += ((score > 0).float() == label).sum()
                total += loss.detach() * label.numel()
            pairs += label.numel()
            edges += n_edges
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        loss_avg, acc = float(total) / pairs, float(correct) / pairs
        how = ("per mini-batch, torch ops" if args.per_batch else f"one step per {args.group} mini-batches")
        print(f"epoch {epoch}: loss {loss_avg:.4f}  link accuracy {acc:.3f}  {dt * 1e3:.1f} ms  {edges} temporal edges sampled, "
              f"{edges / dt / 1e6:.1f} M/s (negatives + sampling + forward + head + backward + Adam; {how})")
        LAST_EPOCH.update(sampled_edges=edges, sampled_edges_per_s=edges / dt, seconds=dt, pairs=pairs)
    return loss_avg, acc


if __name__ == "__main__":
    main()
