#!/usr/bin/env python
"""A Heterogeneous Graph Transformer (PyG's HGTConv) through the package's call groups, on the planted bipartite-plus-self graph of
examples/hetero_transformer_call_groups.py: items carry almost no signal of their class, the USERS that rate them do — so the
model has to read `user -rates-> item`, and the softmax over the edges of `rates` and `similar` TOGETHER decides how much of an
item's row comes from its users.

  * `loader.call_groups()` -> `HeteroCallGroup` -> 2 x `wholegraph_amd.nn.HGTConv`; `x_dict` stays a dict of `LazyRows`; every
    (hop, destination type) of a layer is ONE kernel launch whatever the number of relations ending in the type, forward, and
    two atomic-free kernels backward;
  * one optimizer step per call group, loss printed per epoch, accuracy on held-out items at the end;
  * `--torch-ops` runs the same model out of torch ops (a concatenated edge list, [E, H] logits, a scattered softmax);
  * `--time N` instead times N training steps of BOTH routes on the same call group, alternating, and prints the medians.

    python examples/hgt_call_groups.py [--items 40000] [--epochs 3] [--torch-ops | --time 20]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cugraph-gnn_amd")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from cugraph_pyg_amd.data import FeatureStore, GraphStore  # noqa: E402
from cugraph_pyg_amd.loader import NeighborLoader  # noqa: E402
from wholegraph_amd import nn  # noqa: E402

F_ITEM, F_USER, HIDDEN, HEADS = 64, 96, 64, 4
ETYPES = [("user", "rates", "item"), ("item", "similar", "item"), ("item", "rev_rates", "user")]


def planted_graph(I, U, C, dev):
    """Every item has ~4 ratings, 60 % of them by users of the item's class; users carry their class in their features."""
    g = torch.Generator(device=dev).manual_seed(0)
    item_class = torch.randint(0, C, (I,), generator=g, device=dev)
    user_class = torch.randint(0, C, (U,), generator=g, device=dev)
    n_r = 4 * I
    r_item = torch.arange(n_r, device=dev) % I
    pick = torch.randint(0, U, (n_r,), generator=g, device=dev)
    by_class = torch.argsort(user_class, stable=True)
    first = torch.searchsorted(user_class[by_class], torch.arange(C + 1, device=dev))
    want = item_class[r_item]
    span = (first[want + 1] - first[want]).clamp_(min=1)
    same = by_class[(first[want] + (torch.rand(n_r, generator=g, device=dev) * span).long()).clamp_(max=U - 1)]
    r_user = torch.where(torch.rand(n_r, generator=g, device=dev) < 0.6, same, pick)
    s_src, s_dst = torch.randint(0, I, (3 * I,), generator=g, device=dev), torch.randint(0, I, (3 * I,), generator=g, device=dev)
    gs, fs = GraphStore(), FeatureStore()
    gs[ETYPES[0], "coo", False, (U, I)] = torch.stack([r_user, r_item])
    gs[ETYPES[2], "coo", False, (I, U)] = torch.stack([r_item, r_user])
    gs[ETYPES[1], "coo", False, (I, I)] = torch.stack([s_src, s_dst])
    x_user = torch.randn((U, F_USER), generator=g, device=dev)
    x_user[torch.arange(U, device=dev), user_class] += 2.0
    fs["user", "x", None] = x_user
    fs["item", "x", None] = torch.randn((I, F_ITEM), generator=g, device=dev)          # no class signal of its own
    return fs, gs, item_class, torch.randperm(I, generator=g, device=dev)


def seed_rows(grp):
    """Rows of the group's seeds in ``n_id['item']``: every mini-batch's vertex list starts with its seeds."""
    ptr, bp, G = grp.node_ptr["item"].long(), grp.batch_ptr.long(), grp.n_batches
    per = bp[1:G + 1] - bp[:G]
    within = torch.arange(int(bp[G]), device=ptr.device) - torch.repeat_interleave(bp[:G], per)
    return torch.repeat_interleave(ptr[:G], per) + within


def forward(layers, head, grp):
    h = layers[0](grp.x_dict, grp.layer_graph(0), act="relu")
    h = layers[1](h, grp.layer_graph(1), act="relu")
    return head(h["item"])          # rows = the seeds of all mini-batches, in input order


def step(layers, head, opt, grp, item_class):
    y = item_class[grp.n_id["item"][seed_rows(grp)]]
    loss = F.cross_entropy(forward(layers, head, grp), y)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=40_000)
    ap.add_argument("--users", type=int, default=20_000)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--group", type=int, default=4, help="mini-batches per call group (= per optimizer step)")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--max-groups", type=int, default=0, help="stop every epoch after this many call groups (0: all)")
    ap.add_argument("--torch-ops", action="store_true", help="the torch-ops route instead of the one-kernel layer")
    ap.add_argument("--time", type=int, default=0, help="time this many steps of both routes on the same call group, then stop")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X (there is no CPU fallback)"
    dev = torch.device("cuda")
    I, C = args.items, args.classes
    fs, gs, item_class, perm = planted_graph(I, args.users, C, dev)
    train_ids, test_ids = perm[: I // 2], perm[I // 2: I // 2 + 8 * args.batch_size]

    def loader_over(ids, shuffle):
        return NeighborLoader((fs, gs), {et: [10, 5] for et in ETYPES}, input_nodes=("item", ids), batch_size=args.batch_size,
                              shuffle=shuffle, local_seeds_per_call=args.group * args.batch_size)

    torch.manual_seed(0)
    meta = (["user", "item"], ETYPES)
    layers = torch.nn.ModuleList([nn.HGTConv({"user": F_USER, "item": F_ITEM}, HIDDEN, meta, heads=HEADS),
                                  nn.HGTConv(HIDDEN, HIDDEN, meta, heads=HEADS)]).to(dev)
    head = torch.nn.Linear(HIDDEN, C).to(dev)
    opt = torch.optim.Adam(list(layers.parameters()) + list(head.parameters()), lr=0.005)

    def route(torch_ops):
        for layer in layers:
            layer.torch_ops = torch_ops

    if args.time:
        groups = [next(iter(loader_over(train_ids, False).call_groups()))]
        ms = {False: [], True: []}
        for k in range(3 + args.time):               # three warm-up rounds, then alternate the routes on the same group
            for torch_ops in (False, True):
                route(torch_ops)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                step(layers, head, opt, groups[k % len(groups)], item_class)
                b.record()
                b.synchronize()
                if k >= 3:
                    ms[torch_ops].append(a.elapsed_time(b))
        edges = statistics.mean(g.num_edges for g in groups)
        for torch_ops, name in ((False, "one-kernel layer"), (True, "torch ops")):
            v = sorted(ms[torch_ops])
            print("%s: median %.3f ms per training step (min %.3f, max %.3f, %d steps; %.0f sampled edges per group)"
                  % (name, statistics.median(v), v[0], v[-1], len(v), edges))
        return
    route(args.torch_ops)
    losses = []
    for epoch in range(args.epochs):
        t0, edges = time.perf_counter(), 0
        for k, grp in enumerate(loader_over(train_ids, True).call_groups()):
            if args.max_groups and k >= args.max_groups:
                break
            losses.append(float(step(layers, head, opt, grp, item_class).detach()))
            edges += grp.num_edges
        torch.cuda.synchronize()
        print("epoch %d: loss %.4f (first step %.4f), %.2f M sampled edges/s (training, %s, route %s)" % (
            epoch, losses[-1], losses[0], edges / (time.perf_counter() - t0) / 1e6,
            "torch ops" if args.torch_ops else "one-kernel layer", layers[0].route))
    hit = total = 0
    with torch.no_grad():
        for grp in loader_over(test_ids, False).call_groups():
            y = item_class[grp.n_id["item"][seed_rows(grp)]]
            hit += int((forward(layers, head, grp).argmax(1) == y).sum())
            total += int(y.numel())
    acc = hit / max(total, 1)
    print("test accuracy %.3f over %d items (chance %.3f)" % (acc, total, 1.0 / C))
    return losses[-1], acc


if __name__ == "__main__":
    main()
