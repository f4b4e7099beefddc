#!/usr/bin/env python
"""GraphGPS graph classification: an input Linear, `num_layers` x `wholegraph_amd.nn.GPSConv(C, GINConv(Sequential(Linear, ReLU,
Linear)), heads=4)` — local message passing next to multi-head attention inside each graph —, `global_add_pool`, an MLP head and
`cross_entropy`.  The attention runs on the segment attention kernels over the batch's `ptr` (one launch forward, two backward;
no padded batch), the GIN branch is ONE kernel per layer, the pooling one kernel.

The data is the synthetic set of examples/gin_graph_classification.py with graph sizes drawn from [--min-nodes, --max-nodes]
(10 .. 200 by default): two classes that differ in edge density, node features = the one-hot degree.  A mini-batch is a set of
whole graphs concatenated as PyG's `Batch` does.

    python examples/gps_graph_classification.py [--graphs 600] [--epochs 3] [--torch-ops [--device cpu]] [--time N]

`--torch-ops` runs the same model on the same parameters in plain torch ops: `index_add_` for GIN and, for the attention, the
`to_dense_batch` -> `torch.nn.MultiheadAttention(key_padding_mask=...)` -> `h[mask]` formulation — the yardstick of the timing
and of the loss.  `--time N` trains N steps on the first mini-batch five times over after a warm-up, each window closed by a
device synchronise, and prints the median step time with its spread and the batch's graph sizes as one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cugraph-gnn_amd"), os.path.dirname(os.path.abspath(__file__))]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from gin_graph_classification import collate, make_graphs  # noqa: E402


class GPS(torch.nn.Module):
    def __init__(self, in_channels, hidden, classes, num_layers, heads, dropout, torch_ops):
        super().__init__()
        from wholegraph_amd.nn import GINConv, GPSConv
        self.torch_ops, self.heads, self._mha = torch_ops, heads, {}
        self.lin_in = torch.nn.Linear(in_channels, hidden)
        self.convs = torch.nn.ModuleList(
            GPSConv(hidden, GINConv(torch.nn.Sequential(torch.nn.Linear(hidden, hidden), torch.nn.ReLU(), torch.nn.Linear(hidden, hidden))),
                    heads=heads, dropout=dropout) for _ in range(num_layers))
        self.head = torch.nn.Sequential(torch.nn.Linear(hidden, hidden), torch.nn.ReLU(), torch.nn.Linear(hidden, classes))

    def mha(self, conv):
        """A ``torch.nn.MultiheadAttention`` over the layer's own attention parameters (tied, not copied)."""
        if conv not in self._mha:
            m = torch.nn.MultiheadAttention(conv.channels, self.heads, batch_first=True)
            m.in_proj_weight, m.in_proj_bias = conv.attn.in_proj_weight, conv.attn.in_proj_bias
            m.out_proj.weight, m.out_proj.bias = conv.attn.out_proj.weight, conv.attn.out_proj.bias
            self._mha[conv] = m
        return self._mha[conv].train(self.training)

    def layer_torch_ops(self, conv, x, edge_index, batch, ptr):
        """GPSConv restated: GIN by ``index_add_``, the attention over the padded batch."""
        lin1, _, lin2 = conv.conv.nn
        agg = torch.zeros_like(x).index_add_(0, edge_index[1], x[edge_index[0]]) + (1.0 + conv.conv.eps.to(x.dtype)) * x
        h = F.linear(F.relu(F.linear(agg, lin1.weight, lin1.bias)), lin2.weight, lin2.bias)
        h1 = conv.norm1(F.dropout(h, conv.dropout, self.training) + x)
        sizes = ptr[1:] - ptr[:-1]
        pos = torch.arange(x.shape[0], device=x.device) - ptr[batch]
        mask = torch.arange(int(sizes.max()), device=x.device)[None, :] < sizes[:, None]
        dense = x.new_zeros(mask.shape + (x.shape[1],))
        dense[batch, pos] = x                              # to_dense_batch
        h = self.mha(conv)(dense, dense, dense, key_padding_mask=~mask, need_weights=False)[0][mask]
        h2 = conv.norm2(F.dropout(h, conv.dropout, self.training) + x)
        out = h1 + h2
        return conv.norm3(out + conv.mlp(out))

    def forward(self, x, edge_index, batch, ptr):
        from wholegraph_amd.nn import global_add_pool
        n_graphs = ptr.shape[0] - 1
        x = self.lin_in(x)
        if self.torch_ops:
            for conv in self.convs:
                x = self.layer_torch_ops(conv, x, edge_index, batch, ptr)
            pooled = torch.zeros((n_graphs, x.shape[1]), dtype=x.dtype, device=x.device).index_add_(0, batch, x)
        else:
            for conv in self.convs:
                x = conv(x, edge_index, ptr=ptr)
            pooled = global_add_pool(x, batch, size=n_graphs, ptr=ptr)
        return self.head(pooled)


def time_steps(step, n_steps, sync, repeats=5, warmup=5):
    for _ in range(warmup):
        step()
    sync()
    per_step = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(n_steps):
            step()
        sync()
        per_step.append((time.perf_counter() - t0) / n_steps * 1e3)
    per_step.sort()
    return {"ms_per_step_median": per_step[len(per_step) // 2], "ms_per_step_min": per_step[0], "ms_per_step_max": per_step[-1],
            "steps": n_steps, "repeats": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=600)
    ap.add_argument("--min-nodes", type=int, default=10)
    ap.add_argument("--max-nodes", type=int, default=200)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--num-layers", type=int, default=3)
    ap.add_argument("--lr", type=float, default=0.001)
    ap.add_argument("--dropout", type=float, default=0.0)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--train-split", type=float, default=0.9)
    ap.add_argument("--torch-ops", action="store_true", help="plain torch ops: index_add_ and MultiheadAttention over the padded batch")
    ap.add_argument("--time", type=int, default=0, metavar="N", help="time N training steps on the first mini-batch instead of training")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args()
    if not args.torch_ops or args.time:
        assert args.device == "cuda" and torch.cuda.is_available(), "needs an MI355X (or --torch-ops --device cpu, without --time)"
    dev = torch.device(args.device)
    data = tuple(t.to(dev) for t in make_graphs(args.graphs, args.min_nodes, args.max_nodes, seed=0))
    n_train = int(args.train_split * args.graphs)
    torch.manual_seed(0)                                   # (parameters are drawn on the CPU: the same on every route)
    model = GPS(data[0].shape[1], args.hidden, 2, args.num_layers, args.heads, args.dropout, args.torch_ops).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    order = torch.Generator().manual_seed(1)

    def train_step(x, ei, batch, ptr, y):
        loss = F.cross_entropy(model(x, ei, batch, ptr), y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss

    if args.time:
        model.train()
        x, ei, batch, ptr, y, _ = collate(data, torch.randperm(n_train, generator=order)[:args.batch_size].to(dev))
        sizes = (ptr[1:] - ptr[:-1]).sort().values
        res = time_steps(lambda: train_step(x, ei, batch, ptr, y), args.time, torch.cuda.synchronize)
        res.update(route="torch-ops" if args.torch_ops else "kernel", graphs=int(sizes.shape[0]), nodes=int(ptr[-1]), edges=int(ei.shape[1]),
                   graph_nodes_min=int(sizes[0]), graph_nodes_median=int(sizes[sizes.shape[0] // 2]), graph_nodes_max=int(sizes[-1]),
                   hidden=args.hidden, heads=args.heads, layers=args.num_layers)
        print(json.dumps(res))
        return res
    losses = []
    for epoch in range(args.epochs):
        model.train()
        t0, total = time.perf_counter(), 0.0
        perm = torch.randperm(n_train, generator=order).to(dev)
        for at in range(0, n_train, args.batch_size):
            x, ei, batch, ptr, y, _ = collate(data, perm[at:at + args.batch_size])
            total += float(train_step(x, ei, batch, ptr, y).detach()) * y.shape[0]
        losses.append(total / n_train)
        print(f"epoch {epoch}: loss {losses[-1]:.4f}  {time.perf_counter() - t0:.2f} s", flush=True)
    model.eval()
    correct = 0
    with torch.no_grad():
        for at in range(n_train, args.graphs, args.batch_size):
            x, ei, batch, ptr, y, _ = collate(data, torch.arange(at, min(at + args.batch_size, args.graphs), device=dev))
            correct += int((model(x, ei, batch, ptr).argmax(1) == y).sum())
    acc = correct / max(args.graphs - n_train, 1)
    print(f"test accuracy {acc:.4f} over {args.graphs - n_train} graphs")
    print(json.dumps({"first_loss": losses[0], "last_loss": losses[-1], "test_accuracy": acc}))
    return losses, acc


if __name__ == "__main__":
    main()
