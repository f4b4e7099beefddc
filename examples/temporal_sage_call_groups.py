#!/usr/bin/env python
"""GraphSAGE over TEMPORAL neighbour sampling, iterated in call groups: `NeighborLoader(..., time_attr=..., input_time=...)` —
every seed comes with a time, a hop only follows edges whose time passes `temporal_comparison` against the time its vertex was
reached at (the sampling mode of the reference's movielens_mnmg.py, `time_attr="time"`) — and `loader.call_groups()` walks
`local_seeds_per_call` seeds per launch sequence on the temporal hop of the no-host-sync walk
(`wgamd_sample_hop_pyg_temporal_nosync`): every mini-batch of a group is, bit for bit, the sample `for batch in loader` yields.
Two `nn.SAGEConv` layers run over the group's trimmed layer graphs with a lazy `x`; one optimizer step per group.

`--per-batch` runs the same model and the same samples the way a PyG script does, `for batch in loader`: one mini-batch, one
hop at a time through the framework formulation of the temporal hop (a dozen framework ops and two host read-backs per hop).

    python examples/temporal_sage_call_groups.py [--nodes 200000] [--epochs 3] [--per-batch] [--biased]
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
from cugraph_pyg_amd.loader import NeighborLoader  # noqa: E402
from wholegraph_amd import nn as wnn  # noqa: E402
from wholegraph_amd.nn import SAGEConv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200_000)
    ap.add_argument("--avg-degree", type=int, default=25)
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--group", type=int, default=16, help="mini-batches per call group (= per optimizer step)")
    ap.add_argument("--fanout", type=int, nargs="+", default=[25, 10])
    ap.add_argument("--seeds", type=int, default=0, help="training seeds per epoch (0: half the vertices)")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--time-span", type=int, default=1000, help="edge times are uniform in [0, span); seed times sit at the median")
    ap.add_argument("--comparison", default="monotonically_decreasing")
    ap.add_argument("--biased", action="store_true", help="biased temporal sampling (positive edge weights)")
    ap.add_argument("--per-batch", action="store_true", help="`for batch in loader`: one mini-batch and one hop at a time")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X (there is no CPU fallback)"
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    V, E = args.nodes, args.nodes * args.avg_degree
    src = (torch.rand(E, generator=g, device=dev) ** 2 * V).long().clamp_(max=V - 1)
    dst = torch.randint(0, V, (E,), generator=g, device=dev)
    community = torch.arange(V, device=dev) % args.classes
    x = torch.randn((V, args.features), generator=g, device=dev)
    x[torch.arange(V, device=dev), community % args.features] += 1.0
    graph_store, feature_store = GraphStore(), FeatureStore()
    graph_store[("node", "to", "node"), "coo", False, (V, V)] = torch.stack([src, dst])
    feature_store["node", "x", None] = x
    feature_store[("node", "to", "node"), "time", None] = torch.randint(0, args.time_span, (E,), generator=g, device=dev)   # int64
    if args.biased:
        feature_store[("node", "to", "node"), "w", None] = torch.rand(E, generator=g, device=dev) + 0.05
    n_train = args.seeds or V // 2
    train_ids = torch.randperm(V, generator=g, device=dev)[:n_train]
    train_time = torch.full((n_train,), args.time_span // 2, dtype=torch.int64, device=dev)
    loader = NeighborLoader((feature_store, graph_store), num_neighbors=args.fanout, input_nodes=train_ids, input_time=train_time,
                            time_attr="time", weight_attr="w" if args.biased else None, temporal_comparison=args.comparison,
                            batch_size=args.batch_size, shuffle=True, local_seeds_per_call=args.group * args.batch_size)
    L = len(args.fanout)
    dims = [args.features] + [128] * (L - 1) + [args.classes]
    convs = torch.nn.ModuleList(SAGEConv(dims[i], dims[i + 1]) for i in range(L)).to(dev)
    opt = torch.optim.Adam(convs.parameters(), lr=0.01)
    for epoch in range(args.epochs):
        torch.cuda.synchronize()
        t0, total, seen, edges = time.perf_counter(), torch.zeros((), device=dev), 0, 0
        if args.per_batch:
            for batch in loader:
                n_nodes, n_edges = batch.num_sampled_nodes.tolist(), batch.num_sampled_edges.tolist()
                h = batch.x
                for j, conv in enumerate(convs):        # trimmed hop by hop like torch_geometric.utils.trim_to_layer
                    e_keep, n_dst = sum(n_edges[:L - j]), sum(n_nodes[:L - j])
                    h = conv((h, h[:n_dst]), batch.edge_index[:, :e_keep])
                    h = F.relu(h) if j + 1 < L else h
                loss = F.cross_entropy(h[:batch.batch_size], community[batch.n_id[:batch.batch_size]])
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
                total += loss.detach() * batch.batch_size
                seen += batch.batch_size
                edges += batch.edge_index.shape[1]
        else:
            for grp in loader.call_groups():
                h = grp.x                                           # LazyRows: nothing gathered
                for j, conv in enumerate(convs):
                    h = conv(h, grp.layer_graph(j), act="relu" if j + 1 < L else None)
                loss = wnn.cross_entropy(h, community[grp.batch])
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
                total += loss.detach() * grp.num_seeds
                seen += grp.num_seeds
                edges += grp.num_edges
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        route = "for batch in loader" if args.per_batch else f"call groups of {args.group}"
        print(f"epoch {epoch}: {dt * 1e3:.1f} ms  loss {float(total) / max(seen, 1):.4f}  {edges} temporal edges, "
              f"{edges / dt / 1e6:.2f} M sampled edges/s ({route})")
    return float(total) / max(seen, 1)


if __name__ == "__main__":
    main()
