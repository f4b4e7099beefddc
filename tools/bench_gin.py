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

With --batch-norm the same two shapes compare `GINConv(nn.MLP([F, H, N]))` (route "mlp_bn") with
`GINConv(Sequential(Linear, BatchNorm1d, ReLU, Linear))` (route "linear", the library ops behind the one-product kernel) over the
same parameters in one process, the two alternating call by call: training forward, training forward + backward, eval forward,
and both training outputs against the float64 layer at the tests' bar.  Writes <out-dir>/bench_gin_bn.json; a second run with
--append puts the run-to-run spread on record.

    python tools/bench_gin.py --batch-norm [--append] [--trace]   (--trace: bench_gin_bn_kernel_stats.csv)
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


def timed_pair(fa, fb, iters):
    """ms per call of ``fa`` and of ``fb``, the two alternating call by call (HIP events around every call); which of the two
    goes first swaps from one iteration to the next, so neither always runs behind the other's freed buffers."""
    for _ in range(3):
        fa()
        fb()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
    for k, (s, m, e) in enumerate(ev):
        first, second = (fa, fb) if k % 2 == 0 else (fb, fa)
        s.record()
        first()
        m.record()
        second()
        e.record()
    torch.cuda.synchronize()
    t = [0.0, 0.0]
    for k, (s, m, e) in enumerate(ev):
        t[k % 2] += s.elapsed_time(m)
        t[1 - k % 2] += m.elapsed_time(e)
    return t[0] / iters, t[1] / iters


def measure_batch_norm(name, x, lg, Fi, H, N, iters, x_grad):
    """``GINConv(nn.MLP([F, H, N]))`` (route "mlp_bn") against ``GINConv(Sequential(Linear, BatchNorm1d, ReLU, Linear))`` (route
    "linear": the layer kernel's one-product form, then BatchNorm1d, ReLU and Linear as library ops) over the same parameters:
    training forward, training forward + backward, eval forward, and both routes' training outputs against the float64 layer at
    the tests' bar (|err| <= 1e-5 x magnitude sum + 1e-7; the reported figure is the largest err / bar, <= 1 passes)."""
    from wholegraph_amd import nn
    dev = torch.device("cuda")
    torch.manual_seed(0)
    new = nn.GINConv(nn.MLP([Fi, H, N])).to(dev)
    lin1, bn, lin2 = new.nn.lins[0], new.nn.norms[0].module, new.nn.lins[1]
    bn_seq = torch.nn.BatchNorm1d(H).to(dev)
    bn_seq.weight, bn_seq.bias = bn.weight, bn.bias                    # the same Parameters; each route keeps its own running buffers
    seq = nn.GINConv(torch.nn.Sequential(lin1, bn_seq, torch.nn.ReLU(), lin2)).to(dev)
    assert new.route == "mlp_bn" and seq.route == "linear"
    lazy = isinstance(x, nn.LazyRows)
    n_dst = lg.n_rows
    E = sum(int(h.col.shape[0]) for h in lg.hops)
    R = torch.randn((n_dst, N), device=dev)

    def fwd(conv):
        def run():
            with torch.no_grad():
                return conv(x, lg, act="relu")
        return run

    def train(conv):
        def run():
            xi = x if lazy or not x_grad else x.detach().requires_grad_(True)
            conv.zero_grad(set_to_none=True)
            conv(xi, lg, act="relu").backward(R)
        return run

    # both routes against the float64 layer on the same input
    rows = (x.table[x.ids.long()] if lazy else x).double()
    agg = torch.zeros((n_dst, Fi), dtype=torch.float64, device=dev)
    agg_abs = torch.zeros_like(agg)
    for h, sl, _ in nn._hops(lg):
        dst = nn._edge_dst(h.row_ptr, int(h.col.shape[0]), first=sl.start)
        agg.index_add_(0, dst, rows[h.col.long()])
        agg_abs.index_add_(0, dst, rows[h.col.long()].abs())
        agg[sl] += rows[h.self_rows]
        agg_abs[sl] += rows[h.self_rows].abs()
    del rows
    d = lambda t: t.detach().double()      # noqa: E731
    z = agg @ d(lin1.weight).t() + d(lin1.bias)
    z_abs = agg_abs @ d(lin1.weight).abs().t() + d(lin1.bias).abs()
    del agg, agg_abs
    mean, inv = z.mean(0), (z.var(0, unbiased=False) + bn.eps).rsqrt()
    ref = torch.relu(torch.relu((z - mean) * inv * d(bn.weight) + d(bn.bias)) @ d(lin2.weight).t() + d(lin2.bias))
    scale = ((z_abs + mean.abs()) * inv * d(bn.weight).abs() + d(bn.bias).abs()) @ d(lin2.weight).abs().t() + d(lin2.bias).abs()
    del z, z_abs
    bar = 1e-5 * scale + 1e-7
    new.train(), seq.train()
    err_new = float(((fwd(new)().double() - ref).abs() / bar).max())
    err_seq = float(((fwd(seq)().double() - ref).abs() / bar).max())
    del ref, scale, bar
    torch.cuda.empty_cache()
    t_fn, t_fs = timed_pair(fwd(new), fwd(seq), iters)
    t_tn, t_ts = timed_pair(train(new), train(seq), iters)
    new.eval(), seq.eval()
    t_en, t_es = timed_pair(fwd(new), fwd(seq), iters)
    r4 = lambda v: round(v, 4)             # noqa: E731
    return {
        "shape": {"name": name, "F": Fi, "H": H, "N": N, "dst_rows": n_dst, "edges": E, "src_rows": len(x) if lazy else x.shape[0],
                  "hops": len(lg.hops), "tiles": sum((h.n_rows + 15) // 16 for h in lg.hops), "x": "lazy" if lazy else "tensor",
                  "dX": bool(x_grad and not lazy)},
        "train_forward_ms": {"mlp_bn": r4(t_fn), "sequential": r4(t_fs), "speedup": round(t_fs / t_fn, 3)},
        "train_forward_backward_ms": {"mlp_bn": r4(t_tn), "sequential": r4(t_ts), "speedup": round(t_ts / t_tn, 3)},
        "eval_forward_ms": {"mlp_bn": r4(t_en), "sequential": r4(t_es), "speedup": round(t_es / t_en, 3)},
        "train_output_err_over_bar": {"mlp_bn": round(err_new, 4), "sequential": round(err_seq, 4)},
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
    ap.add_argument("--batch-norm", action="store_true",
                    help="GINConv(nn.MLP([F, H, N])) against GINConv(Sequential(Linear, BatchNorm1d, ReLU, Linear)) -> bench_gin_bn.json")
    ap.add_argument("--append", action="store_true", help="with --batch-norm: add the line to bench_gin_bn.json (a second run: the spread)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    results = []
    run = measure_batch_norm if args.batch_norm else measure
    x, lg, Fi, H, N = products_shape(args.group)
    results.append(run("products", x, lg, Fi, H, N, args.iters, x_grad=False))
    del x, lg
    torch.cuda.empty_cache()
    x, lg, Fi, H, N = small_graphs_shape()
    results.append(run("small_graphs", x, lg, Fi, H, N, args.iters, x_grad=True))
    if args.batch_norm:
        line = json.dumps({"metric": "gin_bn_train_forward_backward_ms", "value": results[0]["train_forward_backward_ms"]["mlp_bn"],
                           "unit": "ms", "results": results})
    else:
        line = json.dumps({"metric": "gin_layer_ms", "value": results[0]["kernel_forward_ms"], "unit": "ms", "results": results})
    print(line)
    if args.no_write:
        return
    stem, mode = ("bench_gin_bn", ["--batch-norm"]) if args.batch_norm else ("bench_gin", [])
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, stem + ".json"), "a" if args.batch_norm and args.append else "w") as f:
        f.write(line + "\n")
    if args.trace:
        with tempfile.TemporaryDirectory() as tmp:
            subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "gin", "--",
                                   sys.executable, os.path.abspath(__file__), "--group", str(args.group), "--iters", "3", "--no-write"]
                                  + mode, stdout=subprocess.DEVNULL)
            found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            assert found, "rocprofv3 wrote no kernel_stats.csv"
            shutil.copy(found[0], os.path.join(args.out_dir, stem + "_kernel_stats.csv"))


if __name__ == "__main__":
    main()
