#!/usr/bin/env python
"""The `Encoder` of the reference's flagship example (python/cugraph-pyg/cugraph_pyg/examples/mag_lp_mnmg.py:48-90) as the
reference writes it, under `to_hetero(aggr="sum")`, over heterogeneous call groups:

    x = conv1(x, ei, ea) + lin1(x);  x = norm1(x);  x = dropout(x);  x = x.relu()
    x = conv2(x, ei, ea);            x = norm2(x);  x = dropout(x);  x = x.relu()
    x = lin2(x).relu()

  * conv1 / conv2: `wholegraph_amd.nn.HeteroConv({edge_type: TransformerConv(..., concat=False, edge_dim=2)})`, one kernel launch
    per (hop, destination type);
  * everything between two convs is `wholegraph_amd.nn.HeteroNormDropoutAct(p=0.5)`: ONE launch for all node types of the layer
    (the `+ lin1(x)` term goes in as its `residual`), two in the backward, no dropout mask stored;
  * `--torch-ops` swaps that block for the chain a model would otherwise run per node type: add, `torch.nn.LayerNorm`,
    `torch.nn.Dropout(0.5)`, `relu`.

The graph is the planted one of examples/hetero_transformer_call_groups.py (items carry almost no signal of their class, the
users that rate them do, and a rating's edge attribute says how much its user agrees with the item); the task is its item
classification, with a linear classifier after `lin2(x).relu()`.  Trains the model on the chosen route, then the same model on
the other one, and prints the loss and the device-synchronised ms per epoch of both routes.

    python examples/mag_encoder_call_groups.py [--items 40000] [--epochs 3] [--torch-ops]
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

F_ITEM, F_USER, HIDDEN, HEADS, EDGE_DIM, P_DROP = 64, 96, 64, 2, 2, 0.5
ETYPES = [("user", "rates", "item"), ("item", "similar", "item"), ("item", "rev_rates", "user")]
WIDTH = {"user": F_USER, "item": F_ITEM}


def planted_graph(I, U, C, dev):
    """The stores and the items' classes: every item has ~4 ratings, 60 % of them by users of the item's class; the rating's
    attribute tells which ones."""
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
    perm = torch.randperm(I, generator=g, device=dev)
    return fs, gs, item_class, perm


def output_input_rows(lg, dev):
    """``{type: int64 [n_out]}``: the row of every output row of the layer graph in the layer's input of the same type."""
    rows = {t: torch.zeros(n, dtype=torch.int64, device=dev) for t, n in lg.n_out.items() if n > 0}
    seen = set()
    for r in lg.relations:
        key = (r.hop, r.edge_type[2])
        if key in seen or r.n_rows == 0:
            continue
        seen.add(key)
        if r.out_rows is None:
            rows[r.edge_type[2]] = r.dst_rows
        else:
            rows[r.edge_type[2]][r.out_rows] = r.dst_rows
    return rows


def input_rows(x, rows):
    """``x[rows]`` without gathering the rest of a ``LazyRows`` input."""
    if isinstance(x, nn.LazyRows) and isinstance(x.table, torch.Tensor):
        return x.table[x.ids[rows].long()].float()
    return x[rows]


class TorchBlock(torch.nn.Module):
    """The chain of torch ops per node type that `HeteroNormDropoutAct` replaces."""

    def __init__(self, channels, p):
        super().__init__()
        self.norms = torch.nn.ModuleDict({t: torch.nn.LayerNorm(c) for t, c in channels.items()})
        self.dropout = torch.nn.Dropout(p)

    def forward(self, x_dict, residual_dict=None):
        out = {}
        for t, x in x_dict.items():
            if residual_dict is not None and residual_dict.get(t) is not None:
                x = x + residual_dict[t]
            out[t] = self.dropout(self.norms[t](x)).relu()
        return out


class Encoder(torch.nn.Module):
    def __init__(self, classes, torch_ops):
        super().__init__()
        conv = lambda fin: nn.HeteroConv({et: nn.TransformerConv(  # noqa: E731
            (fin[et[0]], fin[et[2]]), HIDDEN, heads=HEADS, concat=False, edge_dim=EDGE_DIM) for et in ETYPES})
        hidden = {t: HIDDEN for t in WIDTH}
        self.conv1, self.conv2 = conv(WIDTH), conv(hidden)
        self.lin1 = torch.nn.ModuleDict({t: torch.nn.Linear(WIDTH[t], HIDDEN) for t in WIDTH})
        block = (lambda: TorchBlock(hidden, P_DROP)) if torch_ops else (lambda: nn.HeteroNormDropoutAct(hidden, p=P_DROP))
        self.block1, self.block2 = block(), block()
        self.lin2 = torch.nn.Linear(HIDDEN, HIDDEN)
        self.classifier = torch.nn.Linear(HIDDEN, classes)

    def forward(self, grp):
        ea = grp.edge_attr("attr")
        lg0, lg1 = grp.layer_graph(0), grp.layer_graph(1)
        x = grp.x_dict
        h = self.conv1(x, lg0, edge_attr_dict=ea)
        rows = output_input_rows(lg0, next(iter(h.values())).device)
        res = {t: self.lin1[t](input_rows(x[t], rows[t])) for t in h}            # lin1(x) of the layer's output rows
        h = self.block1(h, res)
        h = self.block2(self.conv2(h, lg1, edge_attr_dict=ea))
        return self.classifier(self.lin2(h["item"]).relu())      # rows = the seeds of all mini-batches, in input order


def seed_rows(grp):
    """Rows of the group's seeds in ``n_id['item']``: every mini-batch's vertex list starts with its seeds."""
    ptr = grp.node_ptr["item"].long()
    bp = grp.batch_ptr.long()
    G = grp.n_batches
    per = bp[1:G + 1] - bp[:G]
    start = torch.repeat_interleave(ptr[:G], per)
    within = torch.arange(int(bp[G]), device=ptr.device) - torch.repeat_interleave(bp[:G], per)
    return start + within


def run(args, torch_ops, data):
    """Trains and tests the encoder on one route of the block; the losses, held-out accuracy and ms per epoch."""
    fs, gs, item_class, perm = data
    dev, I, C, batch = item_class.device, args.items, args.classes, args.batch_size
    train_ids, test_ids = perm[: I // 2], perm[I // 2: I // 2 + 8 * batch]

    def loader_over(ids, shuffle):
        return NeighborLoader((fs, gs), {et: [10, 5] for et in ETYPES}, input_nodes=("item", ids), batch_size=batch,
                              shuffle=shuffle, local_seeds_per_call=args.group * batch)

    torch.manual_seed(0)
    model = Encoder(C, torch_ops).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.005)
    route = "torch ops" if torch_ops else "fused block"
    launches = nn.norm_act_launches
    losses, epoch_ms = [], []
    for epoch in range(args.epochs):
        model.train()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k, grp in enumerate(loader_over(train_ids, True).call_groups()):
            if args.max_groups and k >= args.max_groups:
                break
            y = item_class[grp.n_id["item"][seed_rows(grp)]]
            loss = F.cross_entropy(model(grp), y)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        torch.cuda.synchronize()
        epoch_ms.append((time.perf_counter() - t0) * 1e3)
        print("epoch %d: loss %.4f (first step %.4f), %.1f ms (%s)" % (epoch, losses[-1], losses[0], epoch_ms[-1], route))

    # held-out items, every call group run twice: in eval mode the block draws nothing, so the two passes agree bit for bit
    model.eval()
    hit = total = 0
    same = True
    with torch.no_grad():
        for grp in loader_over(test_ids, False).call_groups():
            y = item_class[grp.n_id["item"][seed_rows(grp)]]
            out = model(grp)
            same = same and bool(torch.equal(out, model(grp)))
            hit += int((out.argmax(1) == y).sum())
            total += int(y.numel())
    acc = hit / max(total, 1)
    print("test accuracy %.3f over %d items (chance %.3f); a second eval pass over the same call groups gives %s logits (%s)" % (
        acc, total, 1.0 / C, "the same" if same else "DIFFERENT", route))
    return {"route": route, "losses": losses, "accuracy": acc, "eval_repeatable": same, "epoch_ms": epoch_ms,
            "block_launches": nn.norm_act_launches - launches}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=40_000)
    ap.add_argument("--users", type=int, default=0, help="default: half the items")
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--group", type=int, default=4, help="mini-batches per call group (= per optimizer step)")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--max-groups", type=int, default=0, help="stop every epoch after this many call groups (0: all)")
    ap.add_argument("--torch-ops", action="store_true", help="the model whose results are returned runs LayerNorm / Dropout / "
                    "relu out of torch ops instead of the fused block (the other route is still run after it, for its times)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X (there is no CPU fallback)"
    data = planted_graph(args.items, args.users or args.items // 2, args.classes, torch.device("cuda"))
    res = run(args, args.torch_ops, data)
    other = run(args, not args.torch_ops, data)          # the same model and data on the other route, for the comparison
    for r in sorted((res, other), key=lambda r: r["route"]):
        print("%-11s ms per epoch (device-synchronised; epoch 0 warms up): %s" % (r["route"], ", ".join("%.1f" % t for t in r["epoch_ms"])))
    res["other"] = other
    return res


if __name__ == "__main__":
    main()
