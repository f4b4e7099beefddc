#!/usr/bin/env python
"""PNA graph classification — the model of PyG's examples/pna.py scaled to the synthetic task of gin_graph_classification.py:
`num_layers` x `PNAConv(hidden, hidden, aggregators=[mean, min, max, std], scalers=[identity, amplification, attenuation], deg)` with
`.relu()` after each, `global_add_pool`, then an MLP head and `cross_entropy`.  Every layer is `wholegraph_amd.nn.PNAConv` — ONE
kernel per layer forward (all four statistics out of one walk over a row, the degree scalers, `post_nns` and `lin`).
The `deg` histogram is counted over the training graphs, as PyG's example does.  Data, collation and the epoch loop are those
of gin_graph_classification.py (random graphs of two edge densities, one-hot degree features, whole graphs per mini-batch).

    python examples/pna_graph_classification.py [--graphs 4000] [--epochs 10] [--torch-ops [--device cpu]]

`--torch-ops` runs the same layers out of torch ops (their "torch" route: four scatter passes over the [E, F] messages and the
[n, 13 F] concatenation) — the yardstick of the epoch times in profiles/pna/README.md.  Prints the loss and the time per epoch,
the test accuracy, and one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cugraph-gnn_amd"), os.path.join(ROOT, "examples")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from gin_graph_classification import collate, make_graphs  # noqa: E402


class PNA(torch.nn.Module):
    def __init__(self, in_channels, hidden, classes, num_layers, dropout, deg, torch_ops):
        super().__init__()
        from wholegraph_amd.nn import PNAConv
        self.embed = torch.nn.Linear(in_channels, hidden)
        self.convs = torch.nn.ModuleList(PNAConv(hidden, hidden, ["mean", "min", "max", "std"], ["identity", "amplification", "attenuation"],
                                                 deg) for _ in range(num_layers))
        for conv in self.convs:
            conv.torch_ops = torch_ops
        self.head = torch.nn.Sequential(torch.nn.Linear(hidden, hidden), torch.nn.ReLU(), torch.nn.Dropout(dropout),
                                        torch.nn.Linear(hidden, classes))

    def forward(self, x, edge_index, batch, ptr):
        from wholegraph_amd.nn import global_add_pool
        x = self.embed(x)
        for conv in self.convs:
            x = conv(x, edge_index, act="relu")
        return self.head(global_add_pool(x, batch, size=ptr.shape[0] - 1, ptr=ptr))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=4000)
    ap.add_argument("--min-nodes", type=int, default=8)
    ap.add_argument("--max-nodes", type=int, default=24)
    ap.add_argument("--batch-size", type=int, default=128)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--num-layers", type=int, default=4)
    ap.add_argument("--lr", type=float, default=0.003)
    ap.add_argument("--dropout", type=float, default=0.5)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--train-split", type=float, default=0.9)
    ap.add_argument("--torch-ops", action="store_true", help="the layers' torch route instead of the HIP kernel (the yardstick)")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args()
    if not args.torch_ops:
        assert args.device == "cuda" and torch.cuda.is_available(), "needs an MI355X (or --torch-ops --device cpu)"
    dev = torch.device(args.device)
    data = make_graphs(args.graphs, args.min_nodes, args.max_nodes, seed=0)
    n_train = int(args.train_split * args.graphs)
    train_nodes = int(data[2][n_train])                    # the deg histogram: in-degrees of the training graphs' nodes
    in_deg = torch.bincount(data[1][1], minlength=int(data[2][-1]))[:train_nodes]
    deg = torch.bincount(in_deg)
    data = tuple(t.to(dev) for t in data)
    torch.manual_seed(0)                                   # (parameters are drawn on the CPU: the same on every route)
    model = PNA(data[0].shape[1], args.hidden, 2, args.num_layers, args.dropout, deg, args.torch_ops).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    order = torch.Generator().manual_seed(1)
    losses, times = [], []
    for epoch in range(args.epochs):
        model.train()
        if dev.type == "cuda":
            torch.cuda.synchronize()
        t0, total = time.perf_counter(), 0.0
        perm = torch.randperm(n_train, generator=order).to(dev)
        for at in range(0, n_train, args.batch_size):
            x, ei, batch, ptr, y, _ = collate(data, perm[at:at + args.batch_size])
            loss = F.cross_entropy(model(x, ei, batch, ptr), y)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            total += float(loss.detach()) * y.shape[0]     # (a device read-back: the epoch's clock stops after the last step)
        losses.append(total / n_train)
        times.append(time.perf_counter() - t0)
        print(f"epoch {epoch}: loss {losses[-1]:.4f}  {times[-1]:.3f} s", flush=True)
    model.eval()
    correct = 0
    with torch.no_grad():
        for at in range(n_train, args.graphs, args.batch_size):
            gids = torch.arange(at, min(at + args.batch_size, args.graphs), device=dev)
            x, ei, batch, ptr, y, _ = collate(data, gids)
            correct += int((model(x, ei, batch, ptr).argmax(1) == y).sum())
    acc = correct / max(args.graphs - n_train, 1)
    print(f"test accuracy {acc:.4f} over {args.graphs - n_train} graphs")
    print(json.dumps({"route": model.convs[0].route, "first_loss": losses[0], "last_loss": losses[-1], "test_accuracy": acc,
                      "epoch_seconds": [round(t, 4) for t in times]}))
    return losses, acc


if __name__ == "__main__":
    main()
