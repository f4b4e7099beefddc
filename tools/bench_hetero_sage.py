#!/usr/bin/env python
"""Two HeteroConv({edge type: SAGEConv}) layers over bench_mag's call group (the ogbn-mag-like graph, all 8 edge types, fan-out
[25, 10], B = 1024, G = 128 mini-batches per call group, F_in = 128, x lazy), hidden width 128 and again 256, timed with HIP
events after warm-up as the median over the call groups:
  (a) the one-kernel route (one wgamd_hetero_sage_layer_f32 launch per (hop, destination type)), forward;
  (b) the same layers through the library-ops route (spmm_csr per relation, nn.Linear, index_copy — relation by relation, the
      pieces the package had before the kernel), forward, over rows gathered beforehand (the gather is timed apart);
  (c) forward + backward of both (every parameter's gradient; x lazy, so no input gradient).
The byte model of one (hop, type) launch is
    sum_r E_r (4 F_r + 4 [+ 8 through a node list])  +  n_f (4 F_dst + 8 |R| + 16)  +  4 n_f N
(per edge: the column, the node id and the neighbour row; per frontier entry: its own row, two CSR bounds per relation, its
input row, node id and output row index; the output row), summed over the launches of both layers and set against 8 TB/s.
Prints one JSON line.

    python tools/bench_hetero_sage.py [--groups 20] [--call-group 128]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cugraph-gnn_amd")]
import torch  # noqa: E402

HBM_PEAK = 8e12


def model_bytes(layer, graph, x, N):
    from wholegraph_amd import nn
    groups = {}
    for r in graph.relations:
        groups.setdefault((r.hop, r.edge_type[2]), []).append(r)
    total = 0
    for (hop, dt), mine in groups.items():
        n_f = mine[0].n_rows
        if n_f == 0:
            continue
        rels = [et for et in layer.edge_types if et[2] == dt]
        for r in mine:
            lazy = isinstance(x[r.edge_type[0]], nn.LazyRows)
            total += r.n_edges * (4 * x[r.edge_type[0]].shape[1] + 4 + (8 if lazy else 0))
        total += n_f * (4 * x[dt].shape[1] + 8 * len(rels) + 16) + 4 * n_f * N
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=20, help="timed call groups (>= 20 for the committed numbers)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--call-group", type=int, default=128, help="mini-batches per call group")
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--hidden", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--no-backward", action="store_true")
    args = ap.parse_args()
    import bench_mag as bm
    from wholegraph_amd import nn
    dev = torch.device("cuda", 0)
    graphs, num_nodes = bm.build_mag_like(dev)
    etypes, ntypes = sorted(graphs), sorted(num_nodes)
    g = torch.Generator(device=dev).manual_seed(5)
    tables = {t: torch.rand((num_nodes[t], bm.F_IN), generator=g, device=dev) * 2 - 1 for t in ntypes}
    B, G, n_groups = args.batch_size, args.call_group, args.groups + args.warmup
    reps = -(-n_groups * G * B // num_nodes["paper"])
    order = torch.cat([torch.randperm(num_nodes["paper"], generator=g, device=dev) for _ in range(reps)])[:n_groups * G * B]
    result = {"metric": "hetero_sage_forward_ms", "unit": "ms", "shape": {"G": G, "B": B, "F_in": bm.F_IN, "fanout": [25, 10],
                                                                         "edge_types": len(etypes), "groups": args.groups}}

    def event_ms(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e), out

    for hidden in args.hidden:
        torch.manual_seed(0)
        model = [nn.HeteroConv({et: nn.SAGEConv((fin, fin), hidden) for et in etypes}).to(dev) for fin in (bm.F_IN, hidden)]
        params = [p for m in model for p in m.parameters()]

        def kernel_fwd(grp):
            h = grp.x_dict
            for j, layer in enumerate(model):
                h = layer(h, grp.layer_graph(j), act="relu")
            return h["paper"]

        def library_fwd(grp, x):
            h = x
            for j, layer in enumerate(model):
                h = layer._forward_sage_library(h, grp.layer_graph(j), True)
            return h["paper"]

        def train(fwd):
            for p in params:
                p.grad = None
            out = fwd()
            out.backward(gout[:out.shape[0]])
            return out

        gout = torch.randn((G * B, hidden), generator=g, device=dev)
        t = {k: [] for k in ("kernel_fwd", "library_fwd", "gather", "kernel_train", "library_train")}
        edges, byts, launches, n = [], [], 0, 0
        loader = bm.make_loader(bm.build_mag_like.graph_store, tables, order, B, G)
        for grp in loader.call_groups():
            for j in range(2):
                grp.layer_graph(j)                     # (index preparation: shared by both routes, outside the timings)
            torch.cuda.synchronize()
            with torch.no_grad():
                before = nn.hetero_sage_launches
                ms_a, out_a = event_ms(lambda: kernel_fwd(grp))
                launches = nn.hetero_sage_launches - before
                ms_g, x = event_ms(lambda: {k: v.materialize() for k, v in grp.x_dict.items()})
                ms_b, out_b = event_ms(lambda: library_fwd(grp, x))
                assert nn.hetero_sage_launches - before == launches, "the baseline must not run the kernel"
                if n == 0:
                    err = float((out_a - out_b).abs().max()) / float(out_b.abs().max())
                    assert err < 1e-4, err
            ms_ta = ms_tb = None
            if not args.no_backward:
                for p in params:
                    p.requires_grad_(True)
                ms_ta, _ = event_ms(lambda: train(lambda: kernel_fwd(grp)))
                ms_tb, _ = event_ms(lambda: train(lambda: library_fwd(grp, x)))
                for p in params:
                    p.requires_grad_(False)
                    p.grad = None
            n += 1
            if n <= args.warmup:
                continue
            for k, v in (("kernel_fwd", ms_a), ("library_fwd", ms_b), ("gather", ms_g), ("kernel_train", ms_ta), ("library_train", ms_tb)):
                if v is not None:
                    t[k].append(v)
            edges.append(grp.num_edges)
            byts.append(sum(model_bytes(model[j], grp.layer_graph(j), grp.x_dict if j == 0 else {k: torch.empty((0, hidden)) for k in ntypes},
                                        hidden) for j in range(2)))
            del x, out_a, out_b
        med = {k: statistics.median(v) for k, v in t.items() if v}
        e_med, b_med = statistics.median(edges), statistics.median(byts)
        result["hidden_%d" % hidden] = {
            "kernel_forward_ms": round(med["kernel_fwd"], 3), "library_forward_ms": round(med["library_fwd"], 3),
            "library_over_kernel_forward": round(med["library_fwd"] / med["kernel_fwd"], 3),
            "gather_ms_not_in_library_forward": round(med["gather"], 3), "launches_per_group": launches,
            "sampled_edges_per_group": int(e_med), "kernel_forward_edges_per_s": round(e_med / (med["kernel_fwd"] * 1e-3), 1),
            "model_bytes_per_group": int(b_med), "fraction_of_hbm_peak": round(b_med / HBM_PEAK / (med["kernel_fwd"] * 1e-3), 4),
            "kernel_forward_backward_ms": round(med["kernel_train"], 3) if "kernel_train" in med else None,
            "library_forward_backward_ms": round(med["library_train"], 3) if "library_train" in med else None,
        }
    result["value"] = result["hidden_%d" % args.hidden[0]]["kernel_forward_ms"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
