#!/usr/bin/env python
"""Layer-1 launch of the one-kernel SAGE layer over a float32, a float16 and a bfloat16 feature table (reported, not gated).

Graph: bench.py's RMAT generator with the products parameters (a = 0.57, b = c = 0.19, symmetrised, 25.3 undirected edges per
vertex) at --nodes vertices; one call group of --group mini-batches of 1024 seeds, fan-out [25, 10], from the loader.  The timed
work is the first layer of the model over ``group.layer_graph(0)`` with ``group.x`` read in the kernel through the node list —
its launches are the ones that fetch feature rows (the hop of fan-out 10 over the 26 k frontier rows per mini-batch, and the
seeds' hop of fan-out 25).  Shapes: F = 100 -> 256 (products layer 1) and F = 256 -> 256 (the half-tile shape).

Per table: ms per layer (HIP events around 20 back-to-back layers after 5 warm-up ones), the bytes the byte model gives
    E (e F + 4) + N_dst (e F + 16) + N_dst 4 N          e = bytes per stored feature (4 or 2)
summed over the layer's hops, and that over time as a fraction of the 8 TB/s HBM peak.  One JSON line per (shape, table)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cugraph-gnn_amd")]
import torch  # noqa: E402

HBM_PEAK_GBPS = 8000.0


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def model_bytes(lg, F, N, elem):
    total = 0
    for h in lg.hops:
        E, n = int(h.col.shape[0]), int(h.n_rows)
        total += E * (elem * F + 4) + n * (elem * F + 16) + n * 4 * N
    return total


def main():
    import bench
    from cugraph_pyg_amd.data import FeatureStore, GraphStore
    from cugraph_pyg_amd.loader import NeighborLoader
    from wholegraph_amd import nn
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1 << 20)
    ap.add_argument("--group", type=int, default=16, help="mini-batches of 1024 seeds in the call group")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda")
    V, G, batch, fanout = args.nodes, args.group, 1024, [25, 10]
    n_und = int(V * bench.E_UNDIRECTED / bench.V_PRODUCTS)
    row_ptr, col = bench.rmat_csr(V, n_und, 1, dev)
    dst = torch.repeat_interleave(torch.arange(V, device=dev), row_ptr[1:] - row_ptr[:-1])
    gs = GraphStore()
    gs[("n", "e", "n"), "coo", False, (V, V)] = torch.stack([col, dst])
    n_edges = int(col.shape[0])
    del dst, row_ptr, col
    seeds = torch.randperm(V, generator=torch.Generator(device=dev).manual_seed(2), device=dev)[:G * batch]
    print(json.dumps({"graph": "rmat(products parameters)", "V": V, "E_directed": n_edges, "G": G, "batch": batch, "fanout": fanout}))
    for F, N in ((100, 256), (256, 256)):
        g = torch.Generator(device=dev).manual_seed(F)
        base = torch.randn((V, F), generator=g, device=dev)
        torch.manual_seed(F)
        conv = nn.SAGEConv(F, N).to(dev)
        first = None
        for name in ("float32", "float16", "bfloat16"):
            dtype = getattr(torch, name)
            table = base.to(dtype)
            fs = FeatureStore()
            fs["n", "x", None] = table
            loader = NeighborLoader((fs, gs), fanout, input_nodes=seeds, batch_size=batch, local_seeds_per_call=G * batch,
                                    shuffle=False, random_state=62)
            grp = next(iter(loader.call_groups()))
            x, lg = grp.x, grp.layer_graph(0)
            assert isinstance(x, nn.LazyRows) and x.table.dtype == dtype
            with torch.no_grad():
                out = conv(x, lg, act="relu")
                assert x._rows is None, "the layer gathered the rows: not the one-kernel route"
                ms = timed(lambda: conv(x, lg, act="relu"), args.warmup, args.iters)
            if name == "float32":
                first = ms
            elem = table.element_size()
            gb = model_bytes(lg, F, N, elem) / 1e9
            print(json.dumps({"shape": "%d->%d" % (F, N), "table": name, "ms_per_layer": round(ms, 4), "model_GB": round(gb, 3),
                              "fraction_of_8TBps": round(gb / (ms * 1e-3) / HBM_PEAK_GBPS, 3),
                              "time_vs_float32": round(ms / first, 3),
                              "hops": [{"rows": int(h.n_rows), "edges": int(h.col.shape[0])} for h in lg.hops],
                              "table_GB": round(table.numel() * elem / 1e9, 3), "finite": bool(torch.isfinite(out).all())}))
            del fs, loader, grp, x, lg, table, out
        del base


if __name__ == "__main__":
    main()
