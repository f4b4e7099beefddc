#!/usr/bin/env python
"""Relational GCN node classification trained in CALL GROUPS — the model of the reference's cugraph-pyg example
rgcn_link_class_mnmg.py (two `FastRGCNConv(hidden, hidden, num_relations, num_bases=30)` layers over a trainable node
embedding, the relation of every sampled edge read as `edge_feature_store[("n", "e", "n"), "rel", None][batch.e_id]`), here
2-layer `wholegraph_amd.nn.RGCNConv(num_bases=30)` over a synthetic graph whose labels can only be read through
relation-typed neighbours: an edge j -> i of relation r comes from a node of colour (label(i) + r) mod classes, so the
label is the neighbours' colour shifted back by their relation — the per-relation weights must undo the shift.  The input is
a trainable embedding read as `emb[grp.n_id]` (the reference's `node_emb`); `grp.edge_attr("rel")` gathers the relation ids
of all sampled edges hop-major, every layer is ONE kernel per hop of the group's trimmed layer graph, forward and backward,
and the optimizer steps once per group.

    python examples/rgcn_call_group_training.py [--nodes 100000] [--epochs 3]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cugraph-gnn_amd")]

import torch  # noqa: E402

from cugraph_pyg_amd.data import FeatureStore, GraphStore  # noqa: E402
from cugraph_pyg_amd.loader import NeighborLoader  # noqa: E402
from wholegraph_amd import nn as wnn  # noqa: E402
from wholegraph_amd.nn import RGCNConv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--avg-degree", type=int, default=12)
    ap.add_argument("--relations", type=int, default=8)
    ap.add_argument("--bases", type=int, default=30)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--group", type=int, default=8, help="mini-batches per call group (= per optimizer step)")
    ap.add_argument("--fanout", type=int, nargs="+", default=[10, 5])
    ap.add_argument("--epochs", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X (there is no CPU fallback)"
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    V, E, K, R = args.nodes, args.nodes * args.avg_degree, args.classes, args.relations
    label = torch.randint(0, K, (V,), generator=g, device=dev)
    colour = torch.arange(V, device=dev) % K                     # node j has colour j mod K
    dst = torch.randint(0, V, (E,), generator=g, device=dev)
    rel = torch.randint(0, R, (E,), generator=g, device=dev)
    want = (label[dst] + rel) % K                                # the colour a source of relation r must have
    src = (torch.randint(0, max(V // K, 1), (E,), generator=g, device=dev) * K + want).clamp_(max=V - 1)
    noise = torch.rand(E, generator=g, device=dev) < 0.1         # 10 % of the edges carry no signal
    src = torch.where(noise, torch.randint(0, V, (E,), generator=g, device=dev), src)
    graph_store, feature_store = GraphStore(), FeatureStore()
    graph_store[("node", "to", "node"), "coo", False, (V, V)] = torch.stack([src, dst])
    feature_store["node", "x", None] = torch.zeros((V, 4), device=dev)             # (the model reads emb, not x)
    feature_store[("node", "to", "node"), "rel", None] = rel
    # node embedding: the colour one-hot plus noise, trainable (the reference example's node_emb)
    emb0 = 0.3 * torch.randn((V, args.hidden), generator=g, device=dev)
    emb0[torch.arange(V, device=dev), colour % args.hidden] += 1.0
    emb = torch.nn.Parameter(emb0)
    train_ids = torch.randperm(V, generator=g, device=dev)[: V // 2]
    loader = NeighborLoader((feature_store, graph_store), num_neighbors=args.fanout, input_nodes=train_ids,
                            batch_size=args.batch_size, shuffle=True, local_seeds_per_call=args.group * args.batch_size)
    L = len(args.fanout)
    convs = torch.nn.ModuleList(RGCNConv(args.hidden, args.hidden, R, num_bases=args.bases) for _ in range(L)).to(dev)
    head = torch.nn.Linear(args.hidden, K).to(dev)
    opt = torch.optim.Adam(list(convs.parameters()) + list(head.parameters()) + [emb], lr=0.01)
    for epoch in range(args.epochs):
        t0, total, correct, seen, edges = time.perf_counter(), 0.0, 0, 0, 0
        for grp in loader.call_groups():
            et = grp.edge_attr("rel")                               # relation of every sampled edge, hop-major
            h = emb[grp.n_id]
            for j, conv in enumerate(convs):
                h = conv(h, grp.layer_graph(j), et, act="relu")
            logits = head(h)
            y = label[grp.batch]                                    # labels of the group's seeds, batch-major like h
            loss = wnn.cross_entropy(logits, y)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            total += float(loss.detach()) * grp.num_seeds
            correct += int((logits.argmax(1) == y).sum())
            seen += grp.num_seeds
            edges += grp.num_edges
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"epoch {epoch}: loss {total / seen:.4f}  train acc {correct / seen:.3f}  {edges / dt / 1e6:.1f} M sampled edges/s "
              f"(sampling + forward + backward + Adam, one step per {args.group} mini-batches), {dt:.2f} s")
    return total / seen, correct / seen


if __name__ == "__main__":
    main()
