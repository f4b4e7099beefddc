#!/usr/bin/env python
"""GATv2 node classification trained in CALL GROUPS — a PyG `GAT(..., v2=True)` model moved onto this package: a 2-layer
`wholegraph_amd.nn.GATv2Conv` (features -> 4 x 64 concatenated -> classes, one head averaged) over a synthetic
planted-community graph, in the shape of examples/gcn_call_group_training.py.  `loader.call_groups()` hands out
`local_seeds_per_call` seeds at a time as one block-diagonal graph, the features stay lazy (`grp.x`), every layer is two
library GEMMs (lin_l over the layer's input rows, lin_r over its destination rows) and ONE attention kernel per hop of the
group's trimmed layer graph — forward; two more per hop backward —, ReLU between the layers rides in the kernel, the loss is
`nn.cross_entropy`, and the optimizer steps once per group.

    python examples/gatv2_call_group_training.py [--nodes 200000] [--epochs 3]
    ... --torch-ops                          the same layers out of torch ops (GATv2Conv's "torch" route)
    ... --torch-ops --float64 --device cpu   the accuracy yardstick: float64 torch ops on the CPU, over mini-batches sampled by a
                                             torch restatement of the loader (same fan-outs, without replacement, one
                                             optimizer step per group)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cugraph-gnn_amd")]

import torch  # noqa: E402

from wholegraph_amd import nn as wnn  # noqa: E402
from wholegraph_amd.nn import GATv2Conv  # noqa: E402


def planted_communities(V, avg_degree, features, classes, seed=0):
    """Edges (70 % inside the source's community), features with one raised column per community, labels — made on the host, so
    every device and dtype trains on the same data."""
    g = torch.Generator().manual_seed(seed)
    E = V * avg_degree
    src = (torch.rand(E, generator=g) ** 2 * V).long().clamp_(max=V - 1)
    dst = torch.randint(0, V, (E,), generator=g)
    community = torch.arange(V) % classes
    same = torch.rand(E, generator=g) < 0.7
    peer = (torch.randint(0, max(V // classes, 1), (E,), generator=g) * classes + community[src]).clamp_(max=V - 1)
    dst = torch.where(same, peer, dst)
    x = torch.randn((V, features), generator=g)
    x[torch.arange(V), community % features] += 1.0
    train_ids = torch.randperm(V, generator=g)[: V // 2]
    return src, dst, x, community, train_ids


def host_mini_batch(in_ptr, in_col, local, seeds, fanout, gen):
    """One mini-batch sampled with torch ops (the yardstick's stand-in for the loader): per hop every frontier node keeps
    min(degree, fan-out) of its in-neighbours without replacement, new nodes are numbered behind the known ones and form the
    next frontier.  Returns ``(n_id, hops)``, hops as ``nn.HopGraph`` over the batch's local numbering."""
    nodes, hops, lo = seeds.clone(), [], 0
    local[nodes] = torch.arange(nodes.shape[0])
    for f in fanout:
        frontier = nodes[lo:]
        deg = in_ptr[frontier + 1] - in_ptr[frontier]
        width = max(int(deg.max()) if deg.numel() else 0, 1)
        keys = torch.rand((frontier.shape[0], width), generator=gen)
        keys[torch.arange(width).unsqueeze(0) >= deg.unsqueeze(1)] = 2.0            # (behind the row's end: never picked first)
        k = min(f, width)
        pick = torch.topk(keys, k, dim=1, largest=False).indices
        keep = torch.arange(k).unsqueeze(0) < deg.clamp(max=f).unsqueeze(1)
        picked = in_col[(in_ptr[frontier].unsqueeze(1) + pick)[keep]]
        new = torch.unique(picked[local[picked] < 0])
        local[new] = torch.arange(nodes.shape[0], nodes.shape[0] + new.shape[0])
        row_ptr = torch.zeros(frontier.shape[0] + 1, dtype=torch.int32)
        row_ptr[1:] = torch.cumsum(keep.sum(1), 0)
        hops.append(wnn.HopGraph(row_ptr, local[picked].to(torch.int32), torch.arange(lo, nodes.shape[0])))
        lo, nodes = nodes.shape[0], torch.cat([nodes, new])
    local[nodes] = -1
    return nodes, hops


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200_000)
    ap.add_argument("--avg-degree", type=int, default=20)
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--hidden", type=int, default=64, help="channels per head of the first layer")
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--group", type=int, default=16, help="mini-batches per call group (= per optimizer step)")
    ap.add_argument("--fanout", type=int, nargs="+", default=[25, 10])
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--torch-ops", action="store_true", help="run the layers out of torch ops (GATv2Conv's 'torch' route)")
    ap.add_argument("--float64", action="store_true")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    assert len(args.fanout) == 2, "a 2-layer model"
    dev = torch.device(args.device)
    on_host = dev.type == "cpu"
    if on_host:
        assert args.torch_ops, "the HIP kernels need an MI355X: --device cpu runs with --torch-ops"
    else:
        assert torch.cuda.is_available(), "needs an MI355X (or --torch-ops --device cpu)"
    dtype = torch.float64 if args.float64 else torch.float32
    V, L = args.nodes, 2
    src, dst, x, community, train_ids = planted_communities(V, args.avg_degree, args.features, args.classes)
    community = community.to(dev)
    torch.manual_seed(0)
    convs = torch.nn.ModuleList([GATv2Conv(args.features, args.hidden, heads=args.heads, concat=True),
                                 GATv2Conv(args.heads * args.hidden, args.classes, heads=1, concat=False)]).to(dev).to(dtype)
    for conv in convs:
        conv.torch_ops = args.torch_ops
    opt = torch.optim.Adam(convs.parameters(), lr=0.01)

    def forward(h, layer_graph):
        for j, conv in enumerate(convs):
            h = conv(h, layer_graph(j), act="relu" if j + 1 < L else None)
        return h

    if on_host:
        order = torch.sort(dst, stable=True).indices
        in_ptr = torch.zeros(V + 1, dtype=torch.int64)
        in_ptr[1:] = torch.cumsum(torch.bincount(dst, minlength=V), 0)
        in_col, local, gen = src[order], torch.full((V,), -1, dtype=torch.int64), torch.Generator().manual_seed(1)
        xt = x.to(dtype)

        def groups():
            ids = train_ids[torch.randperm(train_ids.shape[0], generator=gen)]
            per_group = args.group * args.batch_size
            for g0 in range(0, ids.shape[0], per_group):
                outs, seeds_all, edges = [], ids[g0:g0 + per_group], 0
                for b0 in range(0, seeds_all.shape[0], args.batch_size):           # the group's blocks, one mini-batch each
                    n_id, hops = host_mini_batch(in_ptr, in_col, local, seeds_all[b0:b0 + args.batch_size], args.fanout, gen)
                    outs.append(forward(xt[n_id], lambda j: wnn.LayerGraph(hops[:L - j])))
                    edges += sum(int(h.col.shape[0]) for h in hops)
                yield torch.cat(outs), community[seeds_all], edges
    else:
        from cugraph_pyg_amd.data import FeatureStore, GraphStore
        from cugraph_pyg_amd.loader import NeighborLoader
        graph_store, feature_store = GraphStore(), FeatureStore()
        graph_store[("node", "to", "node"), "coo", False, (V, V)] = torch.stack([src, dst]).to(dev)
        feature_store["node", "x", None] = x.to(dev).to(dtype)
        loader = NeighborLoader((feature_store, graph_store), num_neighbors=args.fanout, input_nodes=train_ids.to(dev),
                                batch_size=args.batch_size, shuffle=True, local_seeds_per_call=args.group * args.batch_size)

        def groups():
            for grp in loader.call_groups():
                # (grp.x is LazyRows: the layer gathers the group's rows once)
                yield forward(grp.x, grp.layer_graph), community[grp.batch], grp.num_edges

    losses, ms, acc = [], [], 0.0
    for epoch in range(args.epochs):
        if not on_host:
            torch.cuda.synchronize()
        t0, total, correct, seen, edges = time.perf_counter(), 0.0, 0, 0, 0
        for h, y, n_edges in groups():
            loss = wnn.cross_entropy(h, y)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            total += float(loss.detach()) * y.shape[0]
            correct += int((h.argmax(1) == y).sum())
            seen += y.shape[0]
            edges += n_edges
        if not on_host:
            torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        losses.append(total / seen)
        ms.append(dt * 1e3)
        acc = correct / seen
        print(f"epoch {epoch}: loss {losses[-1]:.4f}  train acc {acc:.3f}  {dt * 1e3:.1f} ms per epoch  {edges / dt / 1e6:.1f} M sampled "
              f"edges/s (sampling + forward + backward + Adam, one step per {args.group} mini-batches)")
    print(json.dumps({"route": convs[0].route, "first_loss": losses[0], "last_loss": losses[-1], "accuracy": acc,
                      "ms_per_epoch": [round(v, 2) for v in ms]}))
    return losses[-1], acc


if __name__ == "__main__":
    main()
