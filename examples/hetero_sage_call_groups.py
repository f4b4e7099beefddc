#!/usr/bin/env python
"""A heterogeneous GraphSAGE through the package's call groups — the message-passing stack of the reference's bipartite examples
(python/cugraph-pyg/cugraph_pyg/examples/movielens_mnmg.py: `SAGEConv((movie_in, user_in), hidden)` per direction;
mag_lp_mnmg.py: `SAGEConv((hidden, hidden), hidden)` under `to_hetero(aggr="sum")`) on a planted bipartite-plus-self graph:
items carry almost no signal of their class, the USERS that rate them do, so the model has to read `user -rates-> item`.

  * `loader.call_groups()` -> `HeteroCallGroup` -> 2 x `wholegraph_amd.nn.HeteroConv({edge_type: SAGEConv((F_src, F_dst), hidden)})`;
    every (hop, destination type) of a layer is ONE kernel launch (the sum over the relations ending in the type is one product),
    forward and backward; `x_dict` stays a dict of `LazyRows` (the first layer reads the feature tables through the group's node
    lists), the two node types have different feature widths;
  * one optimizer step per call group, loss printed per epoch, accuracy on held-out items at the end.

    python examples/hetero_sage_call_groups.py [--items 40000] [--epochs 3]
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
from wholegraph_amd import nn  # noqa: E402

F_ITEM, F_USER, HIDDEN = 64, 96, 128


def forward(layers, head, grp):
    h = grp.x_dict
    for j, layer in enumerate(layers):
        h = layer(h, grp.layer_graph(j), act="relu")
    return head(h["item"])          # rows = the seeds of all mini-batches, in input order


def seed_rows(grp):
    """Rows of the group's seeds in ``n_id['item']``: every mini-batch's vertex list starts with its seeds."""
    ptr = grp.node_ptr["item"].long()
    bp = grp.batch_ptr.long()
    G = grp.n_batches
    per = bp[1:G + 1] - bp[:G]
    start = torch.repeat_interleave(ptr[:G], per)
    within = torch.arange(int(bp[G]), device=ptr.device) - torch.repeat_interleave(bp[:G], per)
    return start + within


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=40_000)
    ap.add_argument("--users", type=int, default=20_000)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--group", type=int, default=4, help="mini-batches per call group (= per optimizer step)")
    ap.add_argument("--epochs", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X (there is no CPU fallback)"
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    I, U, C = args.items, args.users, args.classes
    item_class = torch.randint(0, C, (I,), generator=g, device=dev)
    user_class = torch.randint(0, C, (U,), generator=g, device=dev)
    # every item has ~4 ratings, 85 % of them by users of the item's class
    n_r = 4 * I
    r_item = torch.arange(n_r, device=dev) % I
    pick = torch.randint(0, U, (n_r,), generator=g, device=dev)
    by_class = torch.argsort(user_class, stable=True)
    first = torch.searchsorted(user_class[by_class], torch.arange(C + 1, device=dev))
    want = item_class[r_item]
    span = (first[want + 1] - first[want]).clamp_(min=1)
    same = by_class[(first[want] + (torch.rand(n_r, generator=g, device=dev) * span).long()).clamp_(max=U - 1)]
    r_user = torch.where(torch.rand(n_r, generator=g, device=dev) < 0.85, same, pick)
    s_src, s_dst = torch.randint(0, I, (3 * I,), generator=g, device=dev), torch.randint(0, I, (3 * I,), generator=g, device=dev)
    gs, fs = GraphStore(), FeatureStore()
    gs[("user", "rates", "item"), "coo", False, (U, I)] = torch.stack([r_user, r_item])
    gs[("item", "rev_rates", "user"), "coo", False, (I, U)] = torch.stack([r_item, r_user])
    gs[("item", "similar", "item"), "coo", False, (I, I)] = torch.stack([s_src, s_dst])
    x_user = torch.randn((U, F_USER), generator=g, device=dev)
    x_user[torch.arange(U, device=dev), user_class] += 2.0
    fs["user", "x", None] = x_user
    fs["item", "x", None] = torch.randn((I, F_ITEM), generator=g, device=dev)          # no class signal of its own
    etypes = [("user", "rates", "item"), ("item", "similar", "item"), ("item", "rev_rates", "user")]
    width = {"user": F_USER, "item": F_ITEM}
    perm = torch.randperm(I, generator=g, device=dev)
    train_ids, test_ids = perm[: I // 2], perm[I // 2: I // 2 + 8 * args.batch_size]

    def loader_over(ids, shuffle):
        return NeighborLoader((fs, gs), {et: [10, 5] for et in etypes}, input_nodes=("item", ids), batch_size=args.batch_size,
                              shuffle=shuffle, local_seeds_per_call=args.group * args.batch_size)

    torch.manual_seed(0)
    layers = torch.nn.ModuleList([
        nn.HeteroConv({et: nn.SAGEConv((width[et[0]], width[et[2]]), HIDDEN) for et in etypes}),
        nn.HeteroConv({et: nn.SAGEConv((HIDDEN, HIDDEN), HIDDEN) for et in etypes})]).to(dev)
    head = torch.nn.Linear(HIDDEN, C).to(dev)
    opt = torch.optim.Adam(list(layers.parameters()) + list(head.parameters()), lr=0.01)
    loss = None
    for epoch in range(args.epochs):
        t0, edges = time.perf_counter(), 0
        for grp in loader_over(train_ids, True).call_groups():
            y = item_class[grp.n_id["item"][seed_rows(grp)]]
            loss = F.cross_entropy(forward(layers, head, grp), y)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            edges += grp.num_edges
        torch.cuda.synchronize()
        print("epoch %d: loss %.4f, %.2f M sampled edges/s (training)" % (epoch, float(loss.detach()), edges / (time.perf_counter() - t0) / 1e6))
    hit = total = 0
    with torch.no_grad():
        for grp in loader_over(test_ids, False).call_groups():
            y = item_class[grp.n_id["item"][seed_rows(grp)]]
            out = forward(layers, head, grp)
            hit += int((out.argmax(1) == y).sum())
            total += int(y.numel())
    acc = hit / max(total, 1)
    print("test accuracy %.3f over %d items (chance %.3f)" % (acc, total, 1.0 / C))
    return float(loss.detach()), acc


if __name__ == "__main__":
    main()
