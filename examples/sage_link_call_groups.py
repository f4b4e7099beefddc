#!/usr/bin/env python
"""The link prediction of examples/sage_link_prediction.py (planted-partition graph, seed edges + binary negatives, 2-layer
GraphSAGE encoder, dot-product decoder, BCE), iterated in CALL GROUPS: `LinkNeighborLoader.call_groups()` hands out the
mini-batches the loader samples per library call as one block-diagonal graph with ONE `edge_label_index` over the seed rows of
the last layer's output; the features stay lazy (`grp.x`), every SAGEConv layer is one kernel over the group's trimmed layer
graph, forward and backward, the head is `wholegraph_amd.nn.link_bce_with_logits` — one launch forward, one per side backward,
no float atomics — and the optimizer steps once per group.  The shape of the reference's link-prediction examples
(python/cugraph-pyg/cugraph_pyg/examples/mag_lp_mnmg.py: encoder -> `(h[src] * h[dst]).sum(-1)` -> BCE).

`--decoder mlp` trains the MLP edge decoder of the reference's movielens_mnmg.py / taobao_mnmg.py instead
(`wholegraph_amd.nn.EdgeDecoder`: `lin2(relu(lin1(cat([h[src], h[dst]], -1))))`, its BCE in the decoder's one forward launch
through `EdgeDecoder.loss`), and prints the first step's loss ahead of the epochs.

`--torch-ops` keeps the loop and swaps the head for the torch formulation of either decoder (gathered copies, `index_put`
backward).

    python examples/sage_link_call_groups.py [--nodes 20000] [--epochs 3] [--decoder {dot,mlp}] [--torch-ops]
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
from wholegraph_amd.nn import SAGEConv  # noqa: E402


def planted_partition(V, E, C, dev, g):
    """90 % of the edges stay inside a community; the features are a noisy one-hot of the community."""
    community = torch.arange(V, device=dev) % C
    src = torch.randint(0, V, (E,), generator=g, device=dev)
    inside = torch.rand(E, generator=g, device=dev) < 0.9
    peer = (torch.randint(0, max(V // C, 1), (E,), generator=g, device=dev) * C + community[src]).clamp_(max=V - 1)
    dst = torch.where(inside, peer, torch.randint(0, V, (E,), generator=g, device=dev))
    x = 0.5 * torch.randn((V, 32), generator=g, device=dev)
    x[torch.arange(V, device=dev), community % 32] += 1.0
    return src, dst, x


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=20_000)
    ap.add_argument("--avg-degree", type=int, default=12)
    ap.add_argument("--communities", type=int, default=20)
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--group", type=int, default=16, help="mini-batches per call group (= per optimizer step)")
    ap.add_argument("--fanout", type=int, nargs="+", default=[10, 5])
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--decoder", choices=["dot", "mlp"], default="dot", help="inner product, or the MLP EdgeDecoder")
    ap.add_argument("--torch-ops", action="store_true", help="the head as torch ops instead of the one-kernel head")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs an MI355X (there is no CPU fallback)"
    dev = torch.device("cuda")
    torch.manual_seed(0)
    g = torch.Generator(device=dev).manual_seed(0)
    V, E = args.nodes, args.nodes * args.avg_degree
    src, dst, x = planted_partition(V, E, args.communities, dev, g)
    graph_store, feature_store = GraphStore(), FeatureStore()
    graph_store[("node", "to", "node"), "coo", False, (V, V)] = torch.stack([src, dst])
    feature_store["node", "x", None] = x
    train_edges = torch.randperm(E, generator=g, device=dev)[: E // 4]
    # a mini-batch of B seed edges and B negatives seeds 4 B endpoints
    loader = LinkNeighborLoader((feature_store, graph_store), num_neighbors=args.fanout,
                                edge_label_index=torch.stack([src[train_edges], dst[train_edges]]), batch_size=args.batch_size,
                                neg_sampling=("binary", 1.0), shuffle=True, local_seeds_per_call=args.group * 4 * args.batch_size)
    L = len(args.fanout)
    dims = [32] + [64] * L
    convs = torch.nn.ModuleList(SAGEConv(dims[i], dims[i + 1]) for i in range(L)).to(dev)
    decoder = wnn.EdgeDecoder(dims[-1]).to(dev) if args.decoder == "mlp" else None
    opt = torch.optim.Adam(list(convs.parameters()) + (list(decoder.parameters()) if decoder else []), lr=0.01)

    def torch_scores(h, eli):
        if decoder is None:
            return (h[eli[0]] * h[eli[1]]).sum(-1)
        return decoder.lin2(decoder.lin1(torch.cat([h[eli[0]], h[eli[1]]], dim=-1)).relu()).view(-1)

    loss_avg = acc = 0.0
    first = decoder is not None
    for epoch in range(args.epochs):
        t0, edges, pairs = time.perf_counter(), 0, 0
        total = torch.zeros((), device=dev)               # (device-side running sums: no read-back per step)
        correct = torch.zeros((), device=dev)
        for grp in loader.call_groups():
            h = grp.x                                       # LazyRows: nothing gathered
            for j, conv in enumerate(convs):
                h = conv(h, grp.layer_graph(j), act="relu" if j + 1 < L else None)
            eli, label = grp.edge_label_index, (grp.edge_label > 0).float()
            if args.torch_ops:
                loss = F.binary_cross_entropy_with_logits(torch_scores(h, eli), label)
            elif decoder is not None:
                loss = decoder.loss(h, h, eli, label)
            else:
                loss = wnn.link_bce_with_logits(h, h, eli, label)
            if first:
                print(f"step 0: loss {float(loss.detach()):.9g}")
                first = False
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            with torch.no_grad():
                score = wnn.pair_dot(h.detach(), h.detach(), eli) if decoder is None else decoder(h.detach(), h.detach(), eli)
                correct += ((score > 0).float() == label).sum()
                total += loss.detach() * label.numel()
            pairs += label.numel()
            edges += grp.num_edges
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        loss_avg, acc = float(total) / pairs, float(correct) / pairs
        print(f"epoch {epoch}: loss {loss_avg:.4f}  link accuracy {acc:.3f}  {edges / dt / 1e6:.1f} M sampled edges/s "
              f"(negatives + sampling + forward + {'torch-op' if args.torch_ops else 'one-kernel'} head + backward + Adam, one step "
              f"per {args.group} mini-batches), {dt:.2f} s")
    return loss_avg, acc


if __name__ == "__main__":
    main()
