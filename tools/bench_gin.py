#!/usr/bin/env python
"""The one-kernel GIN layer (GINConv(Sequential(Linear, ReLU, Linear)), act="relu") against a restatement of the same layer in
plain torch ops (a gather of the lazy rows, `index_add_` over the edges, `F.linear`, `relu` — written here, not the module's own
fallback), forward and forward + backward, timed with HIP events at two shapes:

  * "products": layer 1 of a products-shaped call group (bench.py's graph: RMAT with the products sizes, fan-out [25, 10], batch
    1024, G = 188 mini-batches per call group), F = 100 -> H = 256 -> N = 256, x lazy (read through the node list);
  * "small_graphs": a mini-batch of whole small graphs as examples/gin_graph_classification.py concatenates them (16384 graphs
    of 16 nodes, 4 in-edges per node), F = H = N = 64, x a tensor that needs its gradient (a middle layer).

plus the layer kernel's fraction of the 8 TB/s HBM peak by its byte model  E 4F + N_dst (4F + 4N)  (+ N_dst (4F + 4H) for the
kept aggregate and hidden activation when training).  Writes <out-dir>/bench_gin.json and prints it; with --trace it then runs
itself under `rocprofv3 --kernel-trace --stats` in a fresh process and puts the per-kernel table beside it
(bench_gin_kernel_stats.csv).

    python tools/bench_gin.py [--iters 20] [--group 188] [--out-dir profiles/gin] [--trace]
"""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cugraph-gnn_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM_PEAK = 8e12


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


def torch_ops_layer(x, ids, col, edge_dst, self_rows, n_dst, eps, lin1, lin2):
    """The layer in plain torch ops: relu(relu(agg W1^T + b1) W2^T + b2), agg = sum of the neighbour rows + (1 + eps) self row."""
    rows = x if ids is None else x[ids]
    agg = torch.zeros((n_dst, rows.shape[1]), dtype=rows.dtype, device=rows.device).index_add_(0, edge_dst, rows[col])
    agg = agg + (1.0 + eps) * rows[self_rows]
    return F.relu(F.linear(F.relu(F.linear(agg, lin1.weight, lin1.bias)), lin2.weight, lin2.bias))


def measure(name, x, lg, Fi, H, N, iters, x_grad):
    from wholegraph_amd import nn
    dev = torch.device("cuda")
    torch.manual_seed(0)
    conv = nn.GINConv(torch.nn.Sequential(torch.nn.Linear(Fi, H), torch.nn.ReLU(), torch.nn.Linear(H, N))).to(dev)
    assert conv.route == "mlp"
    lin1, lin2 = conv.nn[0], conv.nn[2]
    lazy = isinstance(x, nn.LazyRows)
    n_dst = lg.n_rows
    E = sum(int(h.col.shape[0]) for h in lg.hops)
    # the torch-op restatement's index arrays, made once outside the timing (as the hops' transposes are for the kernel route)
    col = torch.cat([h.col.long() for h in lg.hops])
    self_rows = torch.cat([h.self_rows for h in lg.hops])
    edge_dst = torch.cat([nn._edge_dst(h.row_ptr, int(h.col.shape[0]), first=rows.start) for h, rows, _ in nn._hops(lg)])
    table, ids = (x.table, x.ids.long()) if lazy else (x, None)
    R = torch.randn((n_dst, N), device=dev)

    def kernel_fwd():
        with torch.no_grad():
            return conv(x, lg, act="relu")

    def torch_fwd():
        with torch.no_grad():
            return torch_ops_layer(table, ids, col, edge_dst, self_rows, n_dst, 0.0, lin1, lin2)

    def kernel_train():
        xi = x if lazy or not x_grad else x.detach().requires_grad_(True)
        conv.zero_grad(set_to_none=True)
        conv(xi, lg, act="relu").backward(R)

    def torch_train():
        ti = table if not x_grad else table.detach().requires_grad_(True)
        conv.zero_grad(set_to_none=True)
        torch_ops_layer(ti, ids, col, edge_dst, self_rows, n_dst, 0.0, lin1, lin2).backward(R)

    a, b = kernel_fwd(), torch_fwd()
    max_diff = float((a - b).abs().max())                   # the two routes compute the same layer
    assert max_diff <= 1e-3 * max(1.0, float(b.abs().max())), max_diff
    del a, b
    t_k, t_t = timed(kernel_fwd, iters), timed(torch_fwd, iters)
    t_kt, t_tt = timed(kernel_train, iters), timed(torch_train, iters)
    bytes_fwd = E * 4 * Fi + n_dst * (4 * Fi + 4 * N)
    bytes_train = bytes_fwd + n_dst * (4 * Fi + 4 * H)
    return {
        "shape": {"name": name, "F": Fi, "H": H, "N": N, "dst_rows": n_dst, "edges": E, "src_rows": len(x) if lazy else x.shape[0],
                  "hops": len(lg.hops), "x": "lazy" if lazy else "tensor", "dX": bool(x_grad and not lazy)},
        "kernel_forward_ms": round(t_k, 4), "torch_ops_forward_ms": round(t_t, 4), "forward_speedup": round(t_t / t_k, 2),
        "kernel_forward_backward_ms": round(t_kt, 4), "torch_ops_forward_backward_ms": round(t_tt, 4),
        "forward_backward_speedup": round(t_tt / t_kt, 2),
        "layer_bytes": bytes_fwd, "layer_hbm_fraction_of_8TBps": round(bytes_fwd / (t_k * 1e-3) / HBM_PEAK, 3),
        "layer_train_bytes": bytes_train, "max_abs_diff_vs_torch_ops": max_diff,
    }


def products_shape(group):
    import bench
    from cugraph_pyg_amd.data import FeatureStore, GraphStore
    from cugraph_pyg_amd.loader import NeighborLoader
    dev = torch.device("cuda")
    V, E_und, Fi, _, fanout = bench.WORKLOADS["products"]
    row_ptr, col = bench.rmat_csr(V, E_und, seed=0, device=dev)
    gs, fs = GraphStore(), FeatureStore()
    dst = torch.repeat_interleave(torch.arange(V, device=dev), row_ptr[1:] - row_ptr[:-1])
    gs[("n", "e", "n"), "coo", False, (V, V)] = torch.stack([col.to(torch.int64), dst])
    del dst
    g = torch.Generator(device=dev).manual_seed(0)
    fs["n", "x", None] = torch.rand((V, Fi), generator=g, device=dev)
    seeds = torch.randperm(V, generator=g, device=dev)[:2 * group * bench.BATCH]
    loader = NeighborLoader((fs, gs), fanout, input_nodes=seeds, batch_size=bench.BATCH, shuffle=False, random_state=62,
                            local_seeds_per_call=group * bench.BATCH)
    grp = next(iter(loader.call_groups()))
    return grp.x, grp.layer_graph(0), Fi, bench.HIDDEN, bench.HIDDEN


def small_graphs_shape(n_graphs=16384, nodes=16, in_deg=4, width=64):
    from wholegraph_amd import nn
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1)
    V = n_graphs * nodes
    dst = torch.repeat_interleave(torch.arange(V, device=dev), in_deg)
    src = dst // nodes * nodes + torch.randint(0, nodes, (V * in_deg,), generator=g, device=dev)     # a node of the same graph
    x = torch.randn((V, width), generator=g, device=dev)
    lg = nn._single_hop(torch.stack([src, dst]), V)[0]
    return x, lg, width, width, width


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", type=int, default=188, help="mini-batches per call group of the products shape")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "gin"))
    ap.add_argument("--trace", action="store_true", help="also run under rocprofv3 --kernel-trace --stats (a fresh process)")
    ap.add_argument("--no-write", action="store_true", help="print only (the traced child)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    results = []
    x, lg, Fi, H, N = products_shape(args.group)
    results.append(measure("products", x, lg, Fi, H, N, args.iters, x_grad=False))
    del x, lg
    torch.cuda.empty_cache()
    x, lg, Fi, H, N = small_graphs_shape()
    results.append(measure("small_graphs", x, lg, Fi, H, N, args.iters, x_grad=True))
    line = json.dumps({"metric": "gin_layer_ms", "value": results[0]["kernel_forward_ms"], "unit": "ms", "results": results})
    print(line)
    if args.no_write:
        return
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "bench_gin.json"), "w") as f:
        f.write(line + "\n")
    if args.trace:
        with tempfile.TemporaryDirectory() as tmp:
            subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "gin", "--",
                                   sys.executable, os.path.abspath(__file__), "--group", str(args.group), "--iters", "3", "--no-write"],
                                  stdout=subprocess.DEVNULL)
            found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            assert found, "rocprofv3 wrote no kernel_stats.csv"
            shutil.copy(found[0], os.path.join(args.out_dir, "bench_gin_kernel_stats.csv"))


if __name__ == "__main__":
    main()
