#!/usr/bin/env python
"""The skeleton of the reference's `Classifier` (cugraph-pyg examples/mag_lp_mnmg.py) on a planted homogeneous graph, iterated
in call groups with one optimizer step per group — the dense products AROUND the message-passing layers run as `nn.RowLinear`:

    x0 = paper_norm(paper_lin(x))                  RowLinear(F, H, norm="layer") over the STORED features: `grp.x` is LazyRows over
                                                   a bfloat16 table (`--feat-dtype`), read in place through `n_id` — the [n, F]
                                                   float32 copy of the rows, the largest tensor of a mini-batch, is never written
    h  = conv2(conv1(x0).relu())                   two nn.SAGEConv, one kernel per hop each
    z  = normalize(lin2(h).relu()) + x0[seeds]     RowLinear(H, H, relu=True, norm="l2")(h, add=...): one launch instead of four
                                                   passes over [n, H]
    logits = lin(z)                                RowLinear(H, classes)

`--torch-ops` runs the SAME parameters through torch.nn.functional (a converting gather of the rows, F.linear, F.layer_norm,
F.normalize, +), which is what the model cost before; both routes print their time per epoch.

    python examples/row_linear_projection.py [--nodes 20000] [--epochs 3] [--feat-dtype bfloat16] [--torch-ops]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cugraph-gnn_amd")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from cugraph_pyg_amd.data import FeatureStore, GraphStore  # noqa: E402
from cugraph_pyg_amd.loader import NeighborLoader  # noqa: E402
from wholegraph_amd import nn as wnn  # noqa: E402


class Classifier(torch.nn.Module):
    def __init__(self, features: int, hidden: int, classes: int, torch_ops: bool):
        super().__init__()
        self.torch_ops = torch_ops
        self.proj = wnn.RowLinear(features, hidden, norm="layer")
        self.conv1, self.conv2 = wnn.SAGEConv(hidden, hidden), wnn.SAGEConv(hidden, hidden)
        self.tail = wnn.RowLinear(hidden, hidden, relu=True, norm="l2")
        self.head = wnn.RowLinear(hidden, classes)

    def forward(self, grp):
        lg0, lg1 = grp.layer_graph(0), grp.layer_graph(1)
        seeds = lg0.hops[0].self_rows                       # rows of the group's seeds in grp.x: the input rows of hop 0's outputs
        x = grp.x
        if self.torch_ops:
            rows = x.materialize() if isinstance(x, wnn.LazyRows) else x
            x0 = F.layer_norm(F.linear(rows, self.proj.lin.weight, self.proj.lin.bias), (self.proj.out_channels,),
                              self.proj.norm.weight, self.proj.norm.bias, self.proj.eps)
        else:
            x0 = self.proj(x)
        h = self.conv2(self.conv1(x0, lg0, act="relu"), lg1)
        if self.torch_ops:
            z = F.normalize(F.linear(h, self.tail.lin.weight, self.tail.lin.bias).relu(), p=2, dim=-1) + x0[seeds]
            return F.linear(z, self.head.lin.weight, self.head.lin.bias)
        return self.head(self.tail(h, add=x0[seeds]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=20_000)
    ap.add_argument("--avg-degree", type=int, default=12)
    ap.add_argument("--features", type=int, default=128)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--group", type=int, default=4, help="mini-batches per call group (= per optimizer step)")
    ap.add_argument("--fanout", type=int, nargs=2, default=[10, 5])
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--feat-dtype", choices=["float32", "float16", "bfloat16"], default="bfloat16",
                    help="dtype the feature table is stored in (16-bit: read as it is by the projection's kernel)")
    ap.add_argument("--torch-ops", action="store_true", help="the dense products out of torch.nn.functional instead of nn.RowLinear")
    ap.add_argument("--json", action="store_true", help="print the result as one JSON line at the end")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X (there is no CPU fallback)"
    dev = torch.device("cuda")
    torch.manual_seed(0)
    g = torch.Generator(device=dev).manual_seed(0)
    V, E = args.nodes, args.nodes * args.avg_degree
    src = torch.randint(0, V, (E,), generator=g, device=dev)
    dst = torch.randint(0, V, (E,), generator=g, device=dev)
    community = torch.arange(V, device=dev) % args.classes
    same = torch.rand(E, generator=g, device=dev) < 0.7
    peer = (torch.randint(0, max(V // args.classes, 1), (E,), generator=g, device=dev) * args.classes + community[src]).clamp_(max=V - 1)
    dst = torch.where(same, peer, dst)
    x = torch.randn((V, args.features), generator=g, device=dev)
    x[torch.arange(V, device=dev), community % args.features] += 1.0
    graph_store, feature_store = GraphStore(), FeatureStore()
    graph_store[("node", "to", "node"), "coo", False, (V, V)] = torch.stack([src, dst])
    feature_store["node", "x", None] = x.to(getattr(torch, args.feat_dtype))
    train_ids = torch.randperm(V, generator=g, device=dev)[: V // 2]
    loader = NeighborLoader((feature_store, graph_store), num_neighbors=args.fanout, input_nodes=train_ids,
                            batch_size=args.batch_size, shuffle=True, local_seeds_per_call=args.group * args.batch_size)
    model = Classifier(args.features, args.hidden, args.classes, args.torch_ops).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    launches0 = wnn.row_linear_launches
    losses, epoch_ms, acc = [], [], 0.0
    for epoch in range(args.epochs):
        t0, correct, seen = time.perf_counter(), 0, 0
        for grp in loader.call_groups():
            logits = model(grp)
            y = community[grp.batch]                            # labels of the group's seeds, batch-major like the output
            loss = wnn.cross_entropy(logits, y)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            correct += int((logits.argmax(1) == y).sum())
            seen += grp.num_seeds
        torch.cuda.synchronize()
        epoch_ms.append((time.perf_counter() - t0) * 1e3)
        acc = correct / max(seen, 1)
        print(f"epoch {epoch}: loss {losses[-1]:.4f}  train acc {acc:.3f}  {epoch_ms[-1]:.1f} ms "
              f"({'torch ops' if args.torch_ops else 'RowLinear'}, {args.feat_dtype} features)")
    res = dict(losses=losses, epoch_ms=epoch_ms, accuracy=acc, torch_ops=args.torch_ops,
               row_linear_launches=wnn.row_linear_launches - launches0, routes=[model.proj.route, model.tail.route, model.head.route])
    if args.json:
        print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
