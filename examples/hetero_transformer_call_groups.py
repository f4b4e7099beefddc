#!/usr/bin/env python
"""A heterogeneous graph transformer through the package's call groups — the message-passing stack of the reference's flagship
link-prediction example (python/cugraph-pyg/cugraph_pyg/examples/mag_lp_mnmg.py:53-66, 156: two `TransformerConv(..., edge_dim=...,
concat=False)` layers with LayerNorm / ReLU between them under `to_hetero(aggr="sum")`) on a planted bipartite-plus-self graph:
items carry almost no signal of their class, the USERS that rate them do, and a rating's edge attribute says how much its user
agrees with the item — so the model has to read `user -rates-> item` and gains from attending by the attribute.

  * `loader.call_groups()` -> `HeteroCallGroup` -> 2 x `wholegraph_amd.nn.HeteroConv({edge_type: TransformerConv((F_src, F_dst),
    hidden, heads, concat=False, edge_dim=2)})`; every (hop, destination type) of a layer is ONE kernel launch (the relations'
    attention-weighted rows side by side times one stacked weight), forward and backward; `x_dict` stays a dict of `LazyRows`
    and `edge_attr_dict = grp.edge_attr("attr")` serves both layers (each reads the prefix of its hops);
  * one optimizer step per call group, loss printed per epoch, accuracy on held-out items at the end;
  * `--torch-ops` runs the same model through the library-ops route (PyG's formulation, relation by relation).

    python examples/hetero_transformer_call_groups.py [--items 40000] [--epochs 3] [--torch-ops]
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

F_ITEM, F_USER, HIDDEN, HEADS, EDGE_DIM = 64, 96, 64, 2, 2


def forward(layers, norms, head, grp):
    ea = grp.edge_attr("attr")
    h = layers[0](grp.x_dict, grp.layer_graph(0), edge_attr_dict=ea)
    h = {t: torch.relu(norms[t](v)) for t, v in h.items()}
    h = layers[1](h, grp.layer_graph(1), edge_attr_dict=ea)
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
    ap.add_argument("--max-groups", type=int, default=0, help="stop every epoch after this many call groups (0: all)")
    ap.add_argument("--torch-ops", action="store_true", help="the library-ops route instead of the one-kernel layer")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X (there is no CPU fallback)"
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    I, U, C = args.items, args.users, args.classes
    item_class = torch.randint(0, C, (I,), generator=g, device=dev)
    user_class = torch.randint(0, C, (U,), generator=g, device=dev)
    # every item has ~4 ratings, 60 % of them by users of the item's class; the rating's attribute tells which ones
    n_r = 4 * I
    r_item = torch.arange(n_r, device=dev) % I
    pick = torch.randint(0, U, (n_r,), generator=g, device=dev)
    by_class = torch.argsort(user_class, stable=True)
    first = torch.searchsorted(user_class[by_class], torch.arange(C + 1, device=dev))
    want = item_class[r_item]
    span = (first[want + 1] - first[want]).clamp_(min=1)
    same = by_class[(first[want] + (torch.rand(n_r, generator=g, device=dev) * span).long()).clamp_(max=U - 1)]
    r_user = torch.where(torch.rand(n_r, generator=g, device=dev) < 0.6, same, pick)
    agree = (user_class[r_user] == item_class[r_item]).float()
    rating = torch.stack([agree + 0.3 * torch.randn(n_r, generator=g, device=dev), torch.randn(n_r, generator=g, device=dev)], 1)
    s_src, s_dst = torch.randint(0, I, (3 * I,), generator=g, device=dev), torch.randint(0, I, (3 * I,), generator=g, device=dev)
    gs, fs = GraphStore(), FeatureStore()
    gs[("user", "rates", "item"), "coo", False, (U, I)] = torch.stack([r_user, r_item])
    gs[("item", "rev_rates", "user"), "coo", False, (I, U)] = torch.stack([r_item, r_user])
    gs[("item", "similar", "item"), "coo", False, (I, I)] = torch.stack([s_src, s_dst])
    fs[("user", "rates", "item"), "attr", None] = rating
    fs[("item", "rev_rates", "user"), "attr", None] = rating
    fs[("item", "similar", "item"), "attr", None] = torch.randn((3 * I, EDGE_DIM), generator=g, device=dev)
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
        nn.HeteroConv({et: nn.TransformerConv((width[et[0]], width[et[2]]), HIDDEN, heads=HEADS, concat=False, edge_dim=EDGE_DIM)
                       for et in etypes}),
        nn.HeteroConv({et: nn.TransformerConv((HIDDEN, HIDDEN), HIDDEN, heads=HEADS, concat=False, edge_dim=EDGE_DIM)
                       for et in etypes})]).to(dev)
    for layer in layers:
        layer.transformer_library_ops = args.torch_ops
    norms = torch.nn.ModuleDict({t: torch.nn.LayerNorm(HIDDEN) for t in width}).to(dev)
    head = torch.nn.Linear(HIDDEN, C).to(dev)
    opt = torch.optim.Adam(list(layers.parameters()) + list(norms.parameters()) + list(head.parameters()), lr=0.005)
    loss, losses = None, []
    for epoch in range(args.epochs):
        t0, edges = time.perf_counter(), 0
        for k, grp in enumerate(loader_over(train_ids, True).call_groups()):
            if args.max_groups and k >= args.max_groups:
                break
            y = item_class[grp.n_id["item"][seed_rows(grp)]]
            loss = F.cross_entropy(forward(layers, norms, head, grp), y)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            edges += grp.num_edges
            losses.append(float(loss.detach()))
        torch.cuda.synchronize()
        print("epoch %d: loss %.4f (first step %.4f), %.2f M sampled edges/s (training, %s)" % (
            epoch, losses[-1], losses[0], edges / (time.perf_counter() - t0) / 1e6, "library ops" if args.torch_ops else "one-kernel layer"))
    hit = total = 0
    with torch.no_grad():
        for grp in loader_over(test_ids, False).call_groups():
            y = item_class[grp.n_id["item"][seed_rows(grp)]]
            out = forward(layers, norms, head, grp)
            hit += int((out.argmax(1) == y).sum())
            total += int(y.numel())
    acc = hit / max(total, 1)
    print("test accuracy %.3f over %d items (chance %.3f)" % (acc, total, 1.0 / C))
    return losses[-1], acc


if __name__ == "__main__":
    main()
