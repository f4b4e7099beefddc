#!/usr/bin/env python
"""Heterogeneous link prediction over call groups — the model of the reference's bipartite link examples
(python/cugraph-pyg/cugraph_pyg/examples/movielens_mnmg.py, taobao_mnmg.py: typed seed edges `user -> item` with binary
negatives, a 2-layer heterogeneous GraphSAGE encoder, the two-`Linear` `EdgeDecoder`, BCE) on a planted bipartite graph: users
and items in C communities, `rates` edges mostly inside a community, the reverse edge type and an `item - item` type beside it,
two feature widths.

  * `LinkNeighborLoader.hetero_call_groups()` -> `HeteroLinkCallGroup`: the mini-batches the loader samples per library call as
    one block-diagonal graph; the source endpoints of the seed edges seed `user`, the destination endpoints `item`, and ONE
    `edge_label_index` indexes the rows of the last layer's output of the two types;
  * 2 x `wholegraph_amd.nn.HeteroConv({edge_type: SAGEConv((F_src, F_dst), hidden)})`: every (hop, destination type) of a layer
    is one kernel launch, forward and backward; `x_dict` stays a dict of `LazyRows`;
  * the head is `wholegraph_amd.nn.EdgeDecoder(hidden)` over `(h["user"], h["item"], grp.edge_label_index)`, its BCE in the
    decoder's one forward launch (`EdgeDecoder.loss`); `--decoder dot` trains the inner product instead
    (`nn.link_bce_with_logits`); one optimizer step per call group.

`--torch-ops` keeps the loop and swaps the head for the torch formulation of either decoder.  `--per-batch` is the loop this
replaces: `for batch in loader`, the same parameters applied with torch ops to every mini-batch's `HeteroData`, the torch head.

    python examples/hetero_link_call_groups.py [--users 20000] [--items 15000] [--epochs 3] [--decoder {mlp,dot}] [--torch-ops]
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
RATES, RATED_BY, SIMILAR = ("user", "rates", "item"), ("item", "rated_by", "user"), ("item", "similar", "item")
LAST_EPOCH = {}       # what the last epoch of the last `main` call measured (tools/bench_link_head.py reads it)


def planted_bipartite(U, I, E, C, dev, g):
    """`rates` edges user -> item, 90 % of them inside the user's community; `similar` edges between items of one community;
    the features are noisy one-hots of the community, of a different width per type."""
    cu, ci = torch.arange(U, device=dev) % C, torch.arange(I, device=dev) % C
    user = torch.randint(0, U, (E,), generator=g, device=dev)
    inside = torch.rand(E, generator=g, device=dev) < 0.9
    peer = (torch.randint(0, max(I // C, 1), (E,), generator=g, device=dev) * C + cu[user]).clamp_(max=I - 1)
    item = torch.where(inside, peer, torch.randint(0, I, (E,), generator=g, device=dev))
    a = torch.randint(0, I, (2 * I,), generator=g, device=dev)
    b = (torch.randint(0, max(I // C, 1), (2 * I,), generator=g, device=dev) * C + ci[a]).clamp_(max=I - 1)
    xu = 0.5 * torch.randn((U, F_USER), generator=g, device=dev)
    xu[torch.arange(U, device=dev), cu % F_USER] += 1.0
    xi = 0.5 * torch.randn((I, F_ITEM), generator=g, device=dev)
    xi[torch.arange(I, device=dev), ci % F_ITEM] += 1.0
    return torch.stack([user, item]), torch.stack([a, b]), xu, xi


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
    ap.add_argument("--items", type=int, default=15_000)
    ap.add_argument("--avg-degree", type=int, default=12, help="`rates` edges per user")
    ap.add_argument("--communities", type=int, default=20)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--group", type=int, default=8, help="mini-batches per call group (= per optimizer step)")
    ap.add_argument("--fanout", type=int, nargs=2, default=[10, 5])
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--decoder", choices=["mlp", "dot"], default="mlp", help="the MLP EdgeDecoder, or the inner product")
    ap.add_argument("--torch-ops", action="store_true", help="the head as torch ops instead of the one-kernel head")
    ap.add_argument("--per-batch", action="store_true", help="`for batch in loader` with torch ops: the loop the call groups replace")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs an MI355X (there is no CPU fallback)"
    dev = torch.device("cuda")
    torch.manual_seed(0)
    g = torch.Generator(device=dev).manual_seed(0)
    U, I, E = args.users, args.items, args.users * args.avg_degree
    rates, similar, xu, xi = planted_bipartite(U, I, E, args.communities, dev, g)
    graph_store, feature_store = GraphStore(), FeatureStore()
    graph_store[RATES, "coo", False, (U, I)] = rates
    graph_store[RATED_BY, "coo", False, (I, U)] = rates.flip(0)
    graph_store[SIMILAR, "coo", False, (I, I)] = similar
    feature_store["user", "x", None] = xu
    feature_store["item", "x", None] = xi
    train = torch.randperm(E, generator=g, device=dev)[: E // 4]
    fan = {et: list(args.fanout) for et in (RATES, RATED_BY, SIMILAR)}
    # a mini-batch of B seed edges and B negatives seeds 2 B endpoints of either type
    loader = LinkNeighborLoader((feature_store, graph_store), num_neighbors=fan, edge_label_index=(RATES, rates[:, train]),
                                batch_size=args.batch_size, neg_sampling=("binary", 1.0), shuffle=True,
                                local_seeds_per_call=args.group * 4 * args.batch_size)
    width = {"user": F_USER, "item": F_ITEM}
    layers = torch.nn.ModuleList([
        wnn.HeteroConv({et: wnn.SAGEConv((width[et[0]], width[et[2]]), args.hidden) for et in fan}),
        wnn.HeteroConv({et: wnn.SAGEConv((args.hidden, args.hidden), args.hidden) for et in fan})]).to(dev)
    decoder = wnn.EdgeDecoder(args.hidden).to(dev) if args.decoder == "mlp" else None
    opt = torch.optim.Adam(list(layers.parameters()) + (list(decoder.parameters()) if decoder else []), lr=0.01)

    def torch_scores(hu, hi, eli):
        if decoder is None:
            return (hu[eli[0]] * hi[eli[1]]).sum(-1)
        return decoder.lin2(decoder.lin1(torch.cat([hu[eli[0]], hi[eli[1]]], dim=-1)).relu()).view(-1)

    def group_step(grp):
        h = grp.x_dict                                      # LazyRows: nothing gathered
        for j, layer in enumerate(layers):
            h = layer(h, grp.layer_graph(j), act="relu" if j + 1 < len(layers) else None)
        hu, hi = h["user"], h["item"]                       # rows = the unique endpoints of all mini-batches, per type
        eli, label = grp.edge_label_index, (grp.edge_label > 0).float()
        if args.torch_ops:
            loss = F.binary_cross_entropy_with_logits(torch_scores(hu, hi, eli), label)
        elif decoder is not None:
            loss = decoder.loss(hu, hi, eli, label)
        else:
            loss = wnn.link_bce_with_logits(hu, hi, eli, label)
        with torch.no_grad():
            score = (wnn.pair_dot(hu.detach(), hi.detach(), eli) if decoder is None else decoder(hu.detach(), hi.detach(), eli))
        return loss, score, label, grp.num_edges

    def batch_step(batch):
        h = plain_forward(layers, batch)
        st = batch[RATES]
        eli, label = st.edge_label_index, (st.edge_label > 0).float()
        score = torch_scores(h["user"], h["item"], eli)
        return F.binary_cross_entropy_with_logits(score, label), score.detach(), label, sum(
            int(batch[et].edge_index.shape[1]) for et in fan)

    loss_avg = acc = 0.0
    for epoch in range(args.epochs):
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
        how = ("per mini-batch, torch ops" if args.per_batch else
               f"{'torch-op' if args.torch_ops else 'one-kernel'} {args.decoder} head, one step per {args.group} mini-batches")
        print(f"epoch {epoch}: loss {loss_avg:.4f}  link accuracy {acc:.3f}  {edges / dt / 1e6:.1f} M sampled edges/s "
              f"(negatives + sampling + forward + head + backward + Adam; {how}), {dt:.2f} s")
        LAST_EPOCH.update(sampled_edges_per_s=edges / dt, seconds=dt, pairs=pairs)
    return loss_avg, acc


if __name__ == "__main__":
    main()
