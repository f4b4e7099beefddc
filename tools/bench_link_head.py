#!/usr/bin/env python
"""The link-prediction head (`nn.link_bce_with_logits`, csrc/wg_link.hip) against its torch formulation, on the pairs of one
products-shaped link call group (bench.py's RMAT graph, fan-out [25, 10], 1024 seed edges + 1024 negatives per mini-batch,
G = 188 mini-batches: P = 188 * 2048 pairs over the group's seed rows), C = 64 and 256, timed with HIP events after warm-up:
forward and forward + backward through `nn`, the same as torch ops, and the row-wise endpoint de-duplication per group — the
torch formulation and the kernel of csrc/wg_rows_unique.hip side by side, at [G, 4096] and [G, 2048].  GB by the byte
model of the BCE forward,
    reads P (8 C + 16 + 4)  +  writes 4 P
(two rows, two int64 indices and a label per pair; the coefficient), and its share of the 8 TB/s HBM peak.  Then the example's
loop (examples/sage_link_call_groups.py) in sampled edges/s through `call_groups()` against `for batch in loader`, same run, and
the heterogeneous example's (examples/hetero_link_call_groups.py) through `hetero_call_groups()` against its `--per-batch` loop.
Prints one JSON line.

    python tools/bench_link_head.py [--iters 20] [--nodes 20000]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cugraph-gnn_amd"), os.path.join(ROOT, "examples")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def head_timings(grp, C, iters, gen):
    from wholegraph_amd import nn
    eli, label = grp.edge_label_index, (grp.edge_label > 0).float()
    P = eli.shape[1]
    h = torch.randn((grp.num_seeds, C), generator=gen, device=eli.device, requires_grad=True)

    def kernel_fwd():
        with torch.no_grad():
            return nn.link_bce_with_logits(h, h, eli, label)

    def torch_fwd():
        with torch.no_grad():
            return F.binary_cross_entropy_with_logits((h[eli[0]] * h[eli[1]]).sum(-1), label)

    def kernel_both():
        h.grad = None
        nn.link_bce_with_logits(h, h, eli, label).backward()

    def torch_both():
        h.grad = None
        F.binary_cross_entropy_with_logits((h[eli[0]] * h[eli[1]]).sum(-1), label).backward()

    t = {"kernel_fwd_ms": timed(kernel_fwd, iters), "torch_fwd_ms": timed(torch_fwd, iters),
         "kernel_fwd_bwd_ms": timed(kernel_both, iters), "torch_fwd_bwd_ms": timed(torch_both, iters)}
    gb = (P * (8 * C + 16 + 4) + 4 * P) / 1e9
    out = {k: round(v, 4) for k, v in t.items()}
    out.update(C=C, pairs=P, seed_rows=grp.num_seeds, fwd_GB=round(gb, 4),
               fwd_hbm_fraction_of_8TBps=round(gb / (t["kernel_fwd_ms"] * 1e-3) / 8e3, 3))
    return out


def example_loops(nodes):
    """Sampled edges/s of one epoch (after a warm-up epoch) of the example's task: the call-group loop with the one-kernel
    head, and the per-batch loop of examples/sage_link_prediction.py."""
    import sage_link_call_groups as ex
    import sage_link_prediction as per_batch
    from cugraph_pyg_amd.data import FeatureStore, GraphStore
    from cugraph_pyg_amd.loader import LinkNeighborLoader
    from wholegraph_amd import nn
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    V, E, B, G = nodes, nodes * 12, 512, 16
    src, dst, x = ex.planted_partition(V, E, 20, dev, g)
    gs, fs = GraphStore(), FeatureStore()
    gs[("node", "to", "node"), "coo", False, (V, V)] = torch.stack([src, dst])
    fs["node", "x", None] = x
    train = torch.randperm(E, generator=g, device=dev)[: E // 4]
    loader = LinkNeighborLoader((fs, gs), num_neighbors=[10, 5], edge_label_index=torch.stack([src[train], dst[train]]), batch_size=B,
                                neg_sampling=("binary", 1.0), shuffle=True, local_seeds_per_call=G * 4 * B)
    convs = torch.nn.ModuleList([nn.SAGEConv(32, 64), nn.SAGEConv(64, 64)]).to(dev)
    opt = torch.optim.Adam(convs.parameters(), lr=0.01)

    def group_epoch():
        edges = 0
        for grp in loader.call_groups():
            h = convs[1](convs[0](grp.x, grp.layer_graph(0), act="relu"), grp.layer_graph(1))
            loss = nn.link_bce_with_logits(h, h, grp.edge_label_index, (grp.edge_label > 0).float())
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            edges += grp.num_edges
        return edges

    model = per_batch.Encoder(32, 64).to(dev)
    opt_b = torch.optim.Adam(model.parameters(), lr=0.01)

    def batch_epoch():
        edges = 0
        for batch in loader:
            h = model(batch.x, batch.edge_index)
            eli = batch.edge_label_index
            loss = F.binary_cross_entropy_with_logits((h[eli[0]] * h[eli[1]]).sum(-1), (batch.edge_label > 0).float())
            opt_b.zero_grad()
            loss.backward()
            opt_b.step()
            edges += batch.edge_index.shape[1]
        return edges

    out = {}
    for name, epoch in (("call_groups", group_epoch), ("per_batch", batch_epoch)):
        epoch()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        edges = epoch()
        torch.cuda.synchronize()
        out[name + "_sampled_edges_per_s"] = round(edges / (time.perf_counter() - t0), 1)
    return out


def products_link_group(group):
    """``(grp, loader, generator)``: the first call group of `group` mini-batches of the products-shaped link task (bench.py's RMAT graph,
    fan-out [25, 10], bench.BATCH seed edges + as many negatives per mini-batch)."""
    import bench
    from cugraph_pyg_amd.data import FeatureStore, GraphStore
    from cugraph_pyg_amd.loader import LinkNeighborLoader
    dev = torch.device("cuda")
    V, E_und, _, _, fanout = bench.WORKLOADS["products"]
    B = bench.BATCH
    row_ptr, col = bench.rmat_csr(V, E_und, seed=0, device=dev)
    gs, fs = GraphStore(), FeatureStore()
    dst = torch.repeat_interleave(torch.arange(V, device=dev), row_ptr[1:] - row_ptr[:-1])
    gs[("n", "e", "n"), "coo", False, (V, V)] = torch.stack([col.to(torch.int64), dst])
    g = torch.Generator(device=dev).manual_seed(0)
    pick = torch.randperm(col.shape[0], generator=g, device=dev)[:group * B]
    loader = LinkNeighborLoader((fs, gs), fanout, edge_label_index=torch.stack([col[pick].to(torch.int64), dst[pick]]), batch_size=B,
                                shuffle=False, random_state=62, neg_sampling=("binary", 1.0), local_seeds_per_call=group * 4 * B)
    del dst
    return next(iter(loader.call_groups())), loader, g


def unique_timings(group, S, V, iters, gen):
    """The row-wise endpoint de-duplication of one call group at [group, S] (ids below V): the torch formulation and the kernel
    (csrc/wg_rows_unique.hip) side by side — three rounds of `iters` timed calls each, alternating, after their warm-up; the
    median round and the spread.  Bytes the kernel moves: reads 8 G S, writes 8 G S (local) + 8 U (lists) + 4 G, then the
    compaction reads 8 U + 4 G and writes 12 G S (uniq and batch with their zero tails)."""
    from cugraph_pyg_amd.loader.link_loader import _batched_first_unique_torch
    from wholegraph_amd import graph_ops
    ends = torch.randint(0, V, (group, S), generator=gen, device="cuda")
    want, got = _batched_first_unique_torch(ends, V), graph_ops.rows_first_unique(ends, V)
    assert all(torch.equal(a, b) for a, b in zip(want, got)), "the kernel and the torch formulation disagree"
    rounds = {"torch": [], "kernel": []}
    for _ in range(3):
        rounds["torch"].append(timed(lambda: _batched_first_unique_torch(ends, V), iters))
        rounds["kernel"].append(timed(lambda: graph_ops.rows_first_unique(ends, V), iters))
    U = int(want[1][-1])
    out = {"shape": [group, S], "unique": U, "kernel_GB": round((8 * group * S * 2 + 16 * U + 8 * group + 12 * group * S) / 1e9, 4)}
    for k, v in rounds.items():
        v = sorted(v)
        out.update({k + "_ms": round(v[1], 4), k + "_ms_min_max": [round(v[0], 4), round(v[-1], 4)]})
    return out


def hetero_example_loops():
    """Sampled edges/s of the last of two epochs of examples/hetero_link_call_groups.py at its defaults: through
    `hetero_call_groups()` with the one-kernel MLP head, and through `for batch in loader` with torch ops."""
    import hetero_link_call_groups as ex
    out = {}
    for name, extra in (("hetero_call_groups", []), ("per_batch", ["--per-batch"])):
        ex.main(["--epochs", "2"] + extra)
        out[name + "_sampled_edges_per_s"] = round(ex.LAST_EPOCH["sampled_edges_per_s"], 1)
        out[name + "_epoch_s"] = round(ex.LAST_EPOCH["seconds"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", type=int, default=188, help="mini-batches per call group")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--nodes", type=int, default=20_000, help="vertices of the example's planted-partition graph")
    args = ap.parse_args()
    import bench
    V, B = bench.WORKLOADS["products"][0], bench.BATCH
    grp, loader, g = products_link_group(args.group)
    heads = [head_timings(grp, C, args.iters, g) for C in (64, 256)]
    del grp, loader
    # [G, 4 B]: both endpoints of B positives + B negatives in one list; [G, 2 B]: one endpoint type of a bipartite group
    unique = [unique_timings(args.group, S, V, args.iters, g) for S in (4 * B, 2 * B)]
    print(json.dumps({"metric": "link_head", "group": args.group, "heads": heads, "batched_first_unique": unique,
                      "example": example_loops(args.nodes), "hetero_example": hetero_example_loops()}))


if __name__ == "__main__":
    main()
