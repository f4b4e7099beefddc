#!/usr/bin/env python
"""GIN graph classification — the model of the reference's cugraph-pyg example dist_gin_sg.py: `num_layers` x
`GINConv(MLP([in, hidden, hidden]), train_eps=False)` with `.relu()` after each, `global_add_pool`, then an MLP head and
`cross_entropy`.  Here every layer is `wholegraph_amd.nn.GINConv(Sequential(Linear, ReLU, Linear))` — ONE kernel per layer
forward (aggregate, both products, biases, both ReLUs) — and the pooling is `wholegraph_amd.nn.global_add_pool` over the sorted
batch vector (one kernel, no atomics).  With `--batch-norm` every layer is `GINConv(wholegraph_amd.nn.MLP([in, hidden, hidden]))`,
PyG's `MLP` with its default `norm="batch_norm"` — the layer the reference trains (Linear -> BatchNorm1d -> ReLU -> Linear; route
"mlp_bn": the layer kernel with per-tile statistics, one finalize launch and one fused tail in training, ONE kernel on the folded
weights in eval mode).

The data is synthetic: a few thousand small random graphs of two classes that differ in edge density, node features = the
one-hot degree (padded to a multiple of 4, as the TU datasets without features get `OneHotDegree`).  A mini-batch is a set of
whole graphs concatenated as PyG's `Batch` does: node ids shifted per graph, one COO `edge_index`, a sorted `batch` vector
and its `ptr`.

    python examples/gin_graph_classification.py [--graphs 4000] [--epochs 10] [--batch-norm] [--torch-ops [--float64] [--device cpu]]

`--torch-ops` runs the same model on the same data in plain torch ops (`index_add_`, `F.linear`, `relu`) — the yardstick of
the accuracy (tests/test_gpu_gin_example.py), on any device.  Prints the loss per epoch, the test accuracy, and one JSON line.
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


def make_graphs(n_graphs, min_nodes, max_nodes, seed):
    """Random graphs back to back (CPU, seeded): class 0 has edge density 0.15, class 1 0.30; every undirected edge is stored
    in both directions, graph after graph.  -> (x [V, F] one-hot degree, edge_index [2, E], node_ptr [G + 1], edge_ptr [G + 1],
    y [G])."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, 2, (n_graphs,), generator=g)
    sizes = torch.randint(min_nodes, max_nodes + 1, (n_graphs,), generator=g)
    node_ptr = torch.zeros(n_graphs + 1, dtype=torch.long)
    node_ptr[1:] = torch.cumsum(sizes, 0)
    srcs, dsts, edge_counts = [], [], []
    for k in range(n_graphs):
        n = int(sizes[k])
        upper = torch.triu(torch.rand((n, n), generator=g) < (0.15 + 0.15 * int(y[k])), diagonal=1)
        a, b = torch.nonzero(upper, as_tuple=True)
        srcs.append(torch.cat([a, b]) + node_ptr[k])
        dsts.append(torch.cat([b, a]) + node_ptr[k])
        edge_counts.append(2 * a.shape[0])
    edge_index = torch.stack([torch.cat(srcs), torch.cat(dsts)])
    edge_ptr = torch.zeros(n_graphs + 1, dtype=torch.long)
    edge_ptr[1:] = torch.cumsum(torch.tensor(edge_counts), 0)
    V = int(node_ptr[-1])
    deg = torch.bincount(edge_index[1], minlength=V)
    width = (max_nodes + 3) // 4 * 4                       # degrees 0 .. max_nodes - 1, padded to a multiple of 4
    x = torch.zeros((V, width))
    x[torch.arange(V), deg] = 1.0
    return x, edge_index, node_ptr, edge_ptr, y


def _ranges(starts, counts):
    """The concatenation of arange(starts[k], starts[k] + counts[k])."""
    total = int(counts.sum())
    first = torch.cumsum(counts, 0) - counts
    return torch.repeat_interleave(starts - first, counts, output_size=total) + torch.arange(total, device=starts.device)


def collate(data, gids):
    """The graphs ``gids`` as one mini-batch, PyG ``Batch`` style: (x, edge_index, batch, ptr, y)."""
    x, edge_index, node_ptr, edge_ptr, y = data
    n_nodes, n_edges = node_ptr[gids + 1] - node_ptr[gids], edge_ptr[gids + 1] - edge_ptr[gids]
    ptr = torch.zeros(gids.shape[0] + 1, dtype=torch.long, device=gids.device)
    ptr[1:] = torch.cumsum(n_nodes, 0)
    nodes, edges = _ranges(node_ptr[gids], n_nodes), _ranges(edge_ptr[gids], n_edges)
    shift = torch.repeat_interleave(ptr[:-1] - node_ptr[gids], n_edges, output_size=edges.shape[0])
    batch = torch.repeat_interleave(torch.arange(gids.shape[0], device=gids.device), n_nodes, output_size=nodes.shape[0])
    return x[nodes], edge_index[:, edges] + shift, batch, ptr, y[gids]


class GIN(torch.nn.Module):
    def __init__(self, in_channels, hidden, classes, num_layers, dropout, torch_ops, batch_norm=False):
        super().__init__()
        from wholegraph_amd.nn import MLP, GINConv
        self.torch_ops = torch_ops
        self.convs = torch.nn.ModuleList()
        for _ in range(num_layers):
            if batch_norm:
                mlp = MLP([in_channels, hidden, hidden])
            else:
                mlp = torch.nn.Sequential(torch.nn.Linear(in_channels, hidden), torch.nn.ReLU(), torch.nn.Linear(hidden, hidden))
            self.convs.append(GINConv(mlp, train_eps=False))
            in_channels = hidden
        self.head = torch.nn.Sequential(torch.nn.Linear(hidden, hidden), torch.nn.ReLU(), torch.nn.Dropout(dropout),
                                        torch.nn.Linear(hidden, classes))

    def forward(self, x, edge_index, batch, ptr):
        from wholegraph_amd.nn import global_add_pool
        n_graphs = ptr.shape[0] - 1
        if self.torch_ops:                                 # the same model restated in plain torch ops
            for conv in self.convs:
                agg = torch.zeros_like(x).index_add_(0, edge_index[1], x[edge_index[0]]) + (1.0 + conv.eps.to(x.dtype)) * x
                if isinstance(conv.nn, torch.nn.Sequential):
                    lin1, _, lin2 = conv.nn
                    x = F.relu(F.linear(F.relu(F.linear(agg, lin1.weight, lin1.bias)), lin2.weight, lin2.bias))
                else:                                      # --batch-norm: the MLP's own forward is torch ops
                    x = F.relu(conv.nn(agg))
            pooled = torch.zeros((n_graphs, x.shape[1]), dtype=x.dtype, device=x.device).index_add_(0, batch, x)
        else:
            for conv in self.convs:
                x = conv(x, edge_index, act="relu")        # one kernel: conv(x, edge_index).relu() of the reference's model
            pooled = global_add_pool(x, batch, size=n_graphs, ptr=ptr)
        return self.head(pooled)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=4000)
    ap.add_argument("--min-nodes", type=int, default=8)
    ap.add_argument("--max-nodes", type=int, default=24)
    ap.add_argument("--batch-size", type=int, default=128)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--num-layers", type=int, default=5)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--dropout", type=float, default=0.5)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--train-split", type=float, default=0.9)
    ap.add_argument("--batch-norm", action="store_true", help="layers GINConv(nn.MLP([in, hidden, hidden])): a BatchNorm1d between the Linears")
    ap.add_argument("--torch-ops", action="store_true", help="plain torch ops instead of the HIP layer (the accuracy yardstick)")
    ap.add_argument("--float64", action="store_true", help="with --torch-ops: float64")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args()
    if not args.torch_ops:
        assert args.device == "cuda" and torch.cuda.is_available(), "needs an MI355X (or --torch-ops --device cpu)"
        assert not args.float64, "--float64 goes with --torch-ops"
    dev = torch.device(args.device)
    dtype = torch.float64 if args.float64 else torch.float32
    data = make_graphs(args.graphs, args.min_nodes, args.max_nodes, seed=0)
    data = (data[0].to(dev, dtype),) + tuple(t.to(dev) for t in data[1:])
    n_train = int(args.train_split * args.graphs)
    torch.manual_seed(0)                                   # (parameters are drawn on the CPU: the same on every route)
    model = GIN(data[0].shape[1], args.hidden, 2, args.num_layers, args.dropout, args.torch_ops, args.batch_norm).to(dev, dtype)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    order = torch.Generator().manual_seed(1)
    losses = []
    for epoch in range(args.epochs):
        model.train()
        t0, total = time.perf_counter(), 0.0
        perm = torch.randperm(n_train, generator=order).to(dev)
        for at in range(0, n_train, args.batch_size):
            x, ei, batch, ptr, y = collate(data, perm[at:at + args.batch_size])
            loss = F.cross_entropy(model(x, ei, batch, ptr), y)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            total += float(loss.detach()) * y.shape[0]
        losses.append(total / n_train)
        print(f"epoch {epoch}: loss {losses[-1]:.4f}  {time.perf_counter() - t0:.2f} s", flush=True)
    model.eval()
    correct = 0
    with torch.no_grad():
        for at in range(n_train, args.graphs, args.batch_size):
            gids = torch.arange(at, min(at + args.batch_size, args.graphs), device=dev)
            x, ei, batch, ptr, y = collate(data, gids)
            correct += int((model(x, ei, batch, ptr).argmax(1) == y).sum())
    acc = correct / max(args.graphs - n_train, 1)
    print(f"test accuracy {acc:.4f} over {args.graphs - n_train} graphs")
    print(json.dumps({"first_loss": losses[0], "last_loss": losses[-1], "test_accuracy": acc}))
    return losses, acc


if __name__ == "__main__":
    main()
