#!/usr/bin/env python
"""TransformerConv layer on bench.py's products-shaped call-group hop (RMAT with the products sizes, fan-out [25, 10], batch
1024, G = 188 mini-batches per call group, x lazy, a [E, 1] edge attribute per sampled edge), timed with HIP events:
  * the reference example's layer (mag_lp_mnmg.py: TransformerConv(64, 64, edge_dim=1, heads=1, concat=False)),
  * F = 100 -> N = 256, H = 1, edge_dim = 1 (against the one-kernel SAGE layer on the same hop),
  * the 2-layer training step (64 -> 64 -> 64, edge_dim 1) per call group.
Each layer is timed as a whole module call — the gather of the destination rows and the u / w GEMM over them included — and
reported as a fraction of the floor max(bytes / 8 TB/s, FLOP / 155 TF/s) of its kernel launches, with the byte model
    E (4 + 8 + 4F + 4D)  +  N_dst (4 + 8 + 8 + 4H (F + D) + 4F_dst + 4N)
(per edge: column, the node id, the neighbour row and its attribute; per destination: CSR bound, self row and its node id,
u and w, its own row and the output row; the u / w GEMM over the destination rows is not counted) and the FLOP
    E H (4F + 4D + 2)  +  2 N_dst K N,   K = H ceil4(F + D + 1) + F_dst
(the logits and the weighted sums per edge; the fp32 MFMA product per destination).  The fraction therefore understates the
kernels' own; their times alone are in a kernel trace of this tool (profiles/transformer/).  Prints one JSON line.

    python tools/bench_transformer.py [--groups 4] [--iters 20]
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
    x64 = torch.rand((V, 64), generator=g, device=dev)
    seeds = torch.randperm(V, generator=g, device=dev)[:(args.groups + 2) * args.group * B]
    loader = NeighborLoader((fs, gs), fanout, input_nodes=seeds, batch_size=B, shuffle=False, random_state=62,
                            local_seeds_per_call=args.group * B)
    groups = iter(loader.call_groups())
    grp = next(groups)
    torch.manual_seed(0)
    ea = torch.randn((grp.num_edges, 1), generator=g, device=dev)
    ref = nn.TransformerConv(64, 64, edge_dim=1, heads=1, concat=False).to(dev)
    wide = nn.TransformerConv(F, N, edge_dim=1, heads=1).to(dev)
    sage = nn.SAGEConv(F, N).to(dev)
    lg = grp.layer_graph(0)
    x100, xr = grp.x, nn.LazyRows(x64, grp.n_id)
    n_dst = lg.n_rows
    E = sum(int(h.col.shape[0]) for h in lg.hops)
    hop0 = lg.hops[0]
    with torch.no_grad():
        t_ref = timed(lambda: ref(xr, lg, ea, act="relu"), args.iters)
        t_wide = timed(lambda: wide(x100, lg, ea, act="relu"), args.iters)
        t_sage = timed(lambda: sage(x100, lg, act="relu"), args.iters)

    def floor(Fi, No, H=1, D=1):
        K = H * nn.transformer_block_width(Fi, D) + Fi
        byt = E * (12 + 4 * Fi + 4 * D) + n_dst * (20 + 4 * H * (Fi + D) + 4 * Fi + 4 * No)
        flop = E * H * (4 * Fi + 4 * D + 2) + 2 * n_dst * K * No
        return byt, flop, max(byt / 8e12, flop / 155e12) * 1e3
    b_ref, f_ref, fl_ref = floor(64, 64)
    b_w, f_w, fl_w = floor(F, N)
    # the 2-layer training step per call group (the reference example's layers: 64 -> 64 -> 64, edge_dim 1)
    convs = torch.nn.ModuleList([nn.TransformerConv(64, 64, edge_dim=1, concat=False),
                                 nn.TransformerConv(64, 64, edge_dim=1, concat=False)]).to(dev)
    opt = torch.optim.Adam(convs.parameters(), lr=0.01)
    y_all = torch.randint(0, 64, (V,), generator=g, device=dev)

    def step(gr):
        e = torch.randn((gr.num_edges, 1), generator=g, device=dev)
        h = nn.LazyRows(x64, gr.n_id)
        for j, conv in enumerate(convs):
            h = conv(h, gr.layer_graph(j), e, act="relu" if j == 0 else None)
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
        "metric": "transformer_ref_layer1_ms", "value": round(t_ref, 4), "unit": "ms",
        "shape": {"G": args.group, "dst_rows": n_dst, "edges": E, "src_rows": len(x100), "hop0_rows": hop0.n_rows},
        "ref_layer": {"F": 64, "C": 64, "H": 1, "D": 1, "concat": False, "ms": round(t_ref, 4), "bytes": b_ref, "flop": f_ref,
                      "floor_ms": round(fl_ref, 4), "fraction_of_floor": round(fl_ref / t_ref, 3)},
        "wide_layer": {"F": F, "N": N, "H": 1, "D": 1, "ms": round(t_wide, 4), "bytes": b_w, "flop": f_w,
                       "floor_ms": round(fl_w, 4), "fraction_of_floor": round(fl_w / t_wide, 3)},
        "sage_layer1_ms": round(t_sage, 4), "wide_over_sage": round(t_wide / t_sage, 3),
        "train_step_ms_per_group": round(ms / max(n, 1), 3), "train_groups": n,
        "train_step_sampled_edges_per_s": round(edges / (ms * 1e-3), 1) if ms > 0 else None,
    }))


if __name__ == "__main__":
    main()
