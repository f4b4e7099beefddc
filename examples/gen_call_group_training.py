#!/usr/bin/env python
"""DeeperGCN-style node classification trained in CALL GROUPS: `wholegraph_amd.nn.GENConv` layers (the per-channel softmax
aggregator with a learnt temperature, `learn_t=True`) over the synthetic planted-community graph of
examples/gatv2_call_group_training.py.  `loader.call_groups()` hands out `local_seeds_per_call` seeds at a time as one
block-diagonal graph, the features stay lazy (`grp.x`: the first layer's `lin_src` / `lin_dst` read the table in place through
`linear_rows`), every layer is ONE kernel per hop of the group's trimmed layer graph forward and one per hop backward — no
[E, C] message, exponential or weight array is written —, the ReLU between the layers rides in the kernel, the loss is
`nn.cross_entropy`, and the optimizer steps once per group.

    python examples/gen_call_group_training.py [--nodes 200000] [--layers 2] [--epochs 3]
    ... --torch-ops          the same parameters through GENConv's "torch" route (scatter softmax over [E, C] arrays)
    ... --repeats 5          after the training epochs, time that many more epochs (device-synchronised) and print their median
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cugraph-gnn_amd")]

import torch  # noqa: E402

from gatv2_call_group_training import planted_communities  # noqa: E402
from wholegraph_amd import nn as wnn  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200_000)
    ap.add_argument("--avg-degree", type=int, default=20)
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--layers", type=int, default=2, choices=(2, 3))
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--group", type=int, default=16, help="mini-batches per call group (= per optimizer step)")
    ap.add_argument("--fanout", type=int, nargs="+", default=None, help="one per layer (default 25 10 / 15 10 5)")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=0, help="timed epochs after the training epochs")
    ap.add_argument("--torch-ops", action="store_true", help="run the layers out of torch ops (GENConv's 'torch' route)")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs an MI355X"
    L = args.layers
    fanout = args.fanout or ([15, 10, 5] if L == 3 else [25, 10])
    assert len(fanout) == L, "one fan-out per layer"
    dev = torch.device("cuda")
    V = args.nodes
    src, dst, x, community, train_ids = planted_communities(V, args.avg_degree, args.features, args.classes)
    community = community.to(dev)
    torch.manual_seed(0)
    widths = [args.features] + [args.hidden] * (L - 1) + [args.classes]
    convs = torch.nn.ModuleList([wnn.GENConv(widths[j], widths[j + 1], learn_t=True, bias=True) for j in range(L)]).to(dev)
    for conv in convs:
        conv.torch_ops = args.torch_ops
    opt = torch.optim.Adam(convs.parameters(), lr=0.01)

    from cugraph_pyg_amd.data import FeatureStore, GraphStore
    from cugraph_pyg_amd.loader import NeighborLoader
    graph_store, feature_store = GraphStore(), FeatureStore()
    graph_store[("node", "to", "node"), "coo", False, (V, V)] = torch.stack([src, dst]).to(dev)
    feature_store["node", "x", None] = x.to(dev)
    loader = NeighborLoader((feature_store, graph_store), num_neighbors=fanout, input_nodes=train_ids.to(dev),
                            batch_size=args.batch_size, shuffle=True, local_seeds_per_call=args.group * args.batch_size)

    def epoch():
        torch.cuda.synchronize()
        t0, total, correct, seen, edges = time.perf_counter(), 0.0, 0, 0, 0
        for grp in loader.call_groups():
            h, y = grp.x, community[grp.batch]                     # (grp.x is LazyRows: no layer gathers the group's rows)
            for j, conv in enumerate(convs):
                h = conv(h, grp.layer_graph(j), act="relu" if j + 1 < L else None)
            loss = wnn.cross_entropy(h, y)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            total += float(loss.detach()) * y.shape[0]
            correct += int((h.argmax(1) == y).sum())
            seen += y.shape[0]
            edges += grp.num_edges
        torch.cuda.synchronize()
        return total / seen, correct / seen, (time.perf_counter() - t0) * 1e3, edges

    losses, ms, acc = [], [], 0.0
    for k in range(args.epochs + args.repeats):
        loss, acc, t_ms, edges = epoch()
        losses.append(loss)
        ms.append(t_ms)
        print(f"epoch {k}: loss {loss:.4f}  train acc {acc:.3f}  {t_ms:.1f} ms per epoch  {edges / t_ms / 1e3:.1f} M sampled edges/s "
              f"(sampling + forward + backward + Adam, one step per {args.group} mini-batches)")
    result = {"route": convs[0].route, "first_loss": losses[0], "last_loss": losses[-1], "accuracy": acc,
              "t": [round(float(conv.t), 4) for conv in convs], "ms_per_epoch": [round(v, 2) for v in ms]}
    if args.repeats:
        timed = ms[args.epochs:]
        result.update(timed_epochs=len(timed), median_ms=round(statistics.median(timed), 2), min_ms=round(min(timed), 2),
                      max_ms=round(max(timed), 2))
    print(json.dumps(result))
    return losses[-1], acc


if __name__ == "__main__":
    main()
