#!/usr/bin/env python
"""GCN layer vs the one-kernel SAGE layer on the same products-shaped call-group hop (bench.py's graph: RMAT with the
products sizes, fan-out [25, 10], batch 1024, G = 188 mini-batches per call group, F = 100 -> N = 256, x lazy), timed with
HIP events; plus the GCN layer's fraction of the 8 TB/s HBM peak by its byte model
    E (4F + 8)  +  N_dst (4F + 20)  +  4 N_dst N
(a neighbour row, its column index and its dinv per edge; per destination row its own row, CSR bounds, self row, dinv and
the output row) and the 2-layer GCN training step (forward, cross entropy, backward, Adam) per call group.
Prints one JSON line.

    python tools/bench_gcn.py [--groups 6] [--iters 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cugraph-gnn_amd")]
import torch  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", type=int, default=188, help="mini-batches per call group")
    ap.add_argument("--groups", type=int, default=6, help="call groups of the training-step timing")
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import bench
    from cugraph_pyg_amd.data import FeatureStore, GraphStore
    from cugraph_pyg_amd.loader import NeighborLoader
    from wholegraph_amd import nn
    dev = torch.device("cuda")
    V, E_und, F, C, fanout = bench.WORKLOADS["products"]
    N, B = bench.HIDDEN, bench.BATCH
    row_ptr, col = bench.rmat_csr(V, E_und, seed=0, device=dev)
    gs, fs = GraphStore(), FeatureStore()
    dst = torch.repeat_interleave(torch.arange(V, device=dev), row_ptr[1:] - row_ptr[:-1])
    gs[("n", "e", "n"), "coo", False, (V, V)] = torch.stack([col.to(torch.int64), dst])
    del dst
    g = torch.Generator(device=dev).manual_seed(0)
    fs["n", "x", None] = torch.rand((V, F), generator=g, device=dev)
    seeds = torch.randperm(V, generator=g, device=dev)[:(args.groups + 2) * args.group * B]
    loader = NeighborLoader((fs, gs), fanout, input_nodes=seeds, batch_size=B, shuffle=False, random_state=62,
                            local_seeds_per_call=args.group * B)
    groups = iter(loader.call_groups())
    grp = next(groups)
    torch.manual_seed(0)
    gcn = nn.GCNConv(F, N).to(dev)
    sage = nn.SAGEConv(F, N).to(dev)
    x, lg = grp.x, grp.layer_graph(0)
    n_dst = lg.n_rows
    E = sum(int(h.col.shape[0]) for h in lg.hops)
    with torch.no_grad():
        gcn(x, lg, act="relu")                              # the group's degrees (once per call group), outside the timing
        t_gcn = timed(lambda: gcn(x, lg, act="relu"), args.iters)
        t_sage = timed(lambda: sage(x, lg, act="relu"), args.iters)
    bytes_gcn = E * (4 * F + 8) + n_dst * (4 * F + 20) + 4 * n_dst * N
    # the 2-layer GCN training step per call group (100 -> 256 -> 47)
    convs = torch.nn.ModuleList([nn.GCNConv(F, N), nn.GCNConv(N, C)]).to(dev)
    opt = torch.optim.Adam(convs.parameters(), lr=0.01)
    y_all = torch.randint(0, C, (V,), generator=g, device=dev)

    def step(gr):
        h = gr.x
        for j, conv in enumerate(convs):
            h = conv(h, gr.layer_graph(j), act="relu" if j == 0 else None)
        loss = nn.cross_entropy(h, y_all[gr.batch])
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return gr.num_edges
    step(grp)                                               # warm-up
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms, edges, n = 0.0, 0, 0
    for gr in groups:                                       # (each group's walk is pipelined by the loader; the timing covers
        s.record()                                          #  the step's device work from the group's hand-out on)
        edges += step(gr)
        e.record()
        torch.cuda.synchronize()
        ms += s.elapsed_time(e)
        n += 1
        if n == args.groups:
            break
    print(json.dumps({
        "metric": "gcn_layer1_ms", "value": round(t_gcn, 4), "unit": "ms",
        "shape": {"G": args.group, "F": F, "N": N, "dst_rows": n_dst, "edges": E, "src_rows": len(x)},
        "sage_layer1_ms": round(t_sage, 4), "gcn_over_sage": round(t_gcn / t_sage, 3),
        "gcn_bytes": bytes_gcn, "gcn_hbm_fraction_of_8TBps": round(bytes_gcn / (t_gcn * 1e-3) / 8e12, 3),
        "gcn_train_step_ms_per_group": round(ms / max(n, 1), 3), "train_groups": n,
        "gcn_train_step_sampled_edges_per_s": round(edges / (ms * 1e-3), 1) if ms > 0 else None,
    }))


if __name__ == "__main__":
    main()
