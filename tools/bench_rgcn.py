#!/usr/bin/env python
"""RGCN layer on bench.py's products-shaped call-group hop (RMAT with the products sizes, fan-out [25, 10], batch 1024,
G = 188 mini-batches per call group, x lazy, relation ids uniform random per sampled edge), timed with HIP events:
  * the reference example's layer (rgcn_link_class_mnmg.py: FastRGCNConv(32, 32, R = 535, num_bases = 30)),
  * F = 100 -> N = 256, R = 8 without bases (against the one-kernel SAGE layer's 1.69 ms on the same hop),
  * the per-edge coefficient kernel, and the 2-layer training step (32 -> 32 -> 32, R = 535, B = 30) per call group.
Each layer launch is reported as a fraction of its floor max(bytes / 8 TB/s, FLOP / 155 TF/s), with the byte model
    E (12 + 8 + 4F)  +  N_dst (4 + 8 + 8 + 4F + 4N)
(per edge: column, relation and coefficient, the node id and the neighbour row; per destination: CSR bound, self row, its
node id, its own row and the output row) and the fp32 MFMA FLOP 2 N_dst (B + 1) F N.  Prints one JSON line.

    python tools/bench_rgcn.py [--groups 4] [--iters 20]
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
    ap.add_argument("--groups", type=int, default=4, help="call groups of the training-step timing")
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
    x32 = torch.rand((V, 32), generator=g, device=dev)
    seeds = torch.randperm(V, generator=g, device=dev)[:(args.groups + 2) * args.group * B]
    loader = NeighborLoader((fs, gs), fanout, input_nodes=seeds, batch_size=B, shuffle=False, random_state=62,
                            local_seeds_per_call=args.group * B)
    groups = iter(loader.call_groups())
    grp = next(groups)
    torch.manual_seed(0)
    R_ref, B_ref, R_8 = 535, 30, 8
    et_ref = torch.randint(0, R_ref, (grp.num_edges,), generator=g, device=dev)
    et_8 = torch.randint(0, R_8, (grp.num_edges,), generator=g, device=dev)
    ref = nn.RGCNConv(32, 32, R_ref, num_bases=B_ref).to(dev)
    wide = nn.RGCNConv(F, N, R_8).to(dev)
    sage = nn.SAGEConv(F, N).to(dev)
    lg = grp.layer_graph(0)
    x100, xr = grp.x, nn.LazyRows(x32, grp.n_id)
    n_dst = lg.n_rows
    E = sum(int(h.col.shape[0]) for h in lg.hops)
    hop0 = lg.hops[0]
    with torch.no_grad():
        t_ref = timed(lambda: ref(xr, lg, et_ref, act="relu"), args.iters)      # (coefficients cached on the graph: the layer)
        t_wide = timed(lambda: wide(x100, lg, et_8, act="relu"), args.iters)
        t_sage = timed(lambda: sage(x100, lg, act="relu"), args.iters)
        t_coef = timed(lambda: [nn.rgcn_edge_coef(h.row_ptr, et_ref[:int(h.col.shape[0])], R_ref) for h in lg.hops], args.iters)

    def floor(Fi, No, Bb):
        byt = E * (20 + 4 * Fi) + n_dst * (20 + 4 * Fi + 4 * No)
        flop = 2 * n_dst * (Bb + 1) * Fi * No
        return byt, flop, max(byt / 8e12, flop / 155e12) * 1e3
    b_ref, f_ref, fl_ref = floor(32, 32, B_ref)
    b_w, f_w, fl_w = floor(F, N, R_8)
    # the 2-layer training step per call group (the reference example's layers: 32 -> 32 -> 32, R = 535, B = 30)
    convs = torch.nn.ModuleList([nn.RGCNConv(32, 32, R_ref, num_bases=B_ref), nn.RGCNConv(32, 32, R_ref, num_bases=B_ref)]).to(dev)
    opt = torch.optim.Adam(convs.parameters(), lr=0.01)
    y_all = torch.randint(0, 32, (V,), generator=g, device=dev)

    def step(gr):
        et = torch.randint(0, R_ref, (gr.num_edges,), generator=g, device=dev)
        h = nn.LazyRows(x32, gr.n_id)
        for j, conv in enumerate(convs):
            h = conv(h, gr.layer_graph(j), et, act="relu" if j == 0 else None)
        loss = nn.cross_entropy(h, y_all[gr.batch])
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return gr.num_edges
    step(grp)                                               # warm-up
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms, edges, n = 0.0, 0, 0
    for gr in groups:
        s.record()
        edges += step(gr)
        e.record()
        torch.cuda.synchronize()
        ms += s.elapsed_time(e)
        n += 1
        if n == args.groups:
            break
    print(json.dumps({
        "metric": "rgcn_ref_layer1_ms", "value": round(t_ref, 4), "unit": "ms",
        "shape": {"G": args.group, "dst_rows": n_dst, "edges": E, "src_rows": len(x100), "hop0_rows": hop0.n_rows},
        "ref_layer": {"F": 32, "N": 32, "R": R_ref, "B": B_ref, "ms": round(t_ref, 4), "bytes": b_ref, "flop": f_ref,
                      "floor_ms": round(fl_ref, 4), "fraction_of_floor": round(fl_ref / t_ref, 3)},
        "wide_layer": {"F": F, "N": N, "R": R_8, "B": None, "ms": round(t_wide, 4), "bytes": b_w, "flop": f_w,
                       "floor_ms": round(fl_w, 4), "fraction_of_floor": round(fl_w / t_wide, 3)},
        "sage_layer1_ms": round(t_sage, 4), "wide_over_sage": round(t_wide / t_sage, 3),
        "coef_ms_all_hops": round(t_coef, 4),
        "train_step_ms_per_group": round(ms / max(n, 1), 3), "train_groups": n,
        "train_step_sampled_edges_per_s": round(edges / (ms * 1e-3), 1) if ms > 0 else None,
    }))


if __name__ == "__main__":
    main()
