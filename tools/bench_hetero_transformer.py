#!/usr/bin/env python
"""Time per call group of HeteroConv{TransformerConv} over the ogbn-mag-like workload of bench_mag.py, two routes in one process:

  * grouped  — ``nn.HeteroConv`` over the call group's ``HeteroLayerGraph``: one ``wgamd_hetero_transformer_layer_f32`` launch per
    (hop, destination type);
  * relation — relation by relation, what the package offered before the grouped kernel: per ``RelationHop`` one
    ``TransformerConv((x_src, x_dst[dst_rows]), [row_ptr, col])`` (one ``wgamd_transformer_layer_f32`` launch each) and an
    ``index_add`` into the destination type's rows.

Measured per call group, on call groups fetched before the clock starts (the walk is not part of it): one two-layer forward
(no autograd) and one training step (forward, a fixed linear loss, backward, SGD step).  HIP events around every repetition,
the routes interleaved; prints one JSON line with median / min / max per route and measurement.

    python tools/bench_hetero_transformer.py [--call-group 128] [--batch-size 1024] [--hidden 64] [--heads 1] [--reps 10]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cugraph-gnn_amd")]

import torch  # noqa: E402

import bench_mag as bm  # noqa: E402
from wholegraph_amd import nn  # noqa: E402


def grouped(model, xs, graphs, act):
    h = xs
    for j, layer in enumerate(model):
        h = layer(h, graphs[j], act=act if j == 0 else None)
    return h["paper"]


def relation_by_relation(model, xs, graphs, act):
    h = {t: (v.materialize() if isinstance(v, nn.LazyRows) else v) for t, v in xs.items()}
    for j, layer in enumerate(model):
        graph = graphs[j]
        dev = next(iter(h.values())).device
        out = {t: torch.zeros((n, layer._width(t)), dtype=torch.float32, device=dev) for t, n in graph.n_out.items() if n > 0}
        for r in graph.relations:
            if r.n_rows == 0:
                continue
            et = r.edge_type
            y = layer.conv(et)((h[et[0]], h[et[2]][r.dst_rows]), [r.row_ptr, r.col])
            rows = r.out_rows if r.out_rows is not None else torch.arange(r.n_rows, device=dev)
            out[et[2]] = out[et[2]].index_add(0, rows, y)
        h = {t: torch.relu(v) for t, v in out.items()} if (act == "relu" and j == 0) else out
    return h["paper"]


def timed(fn, reps, warm):
    times = []
    for k in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k >= warm:
            times.append(a.elapsed_time(b))
    return times


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3), "reps": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--call-group", type=int, default=128)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--heads", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--groups", type=int, default=2, help="call groups the repetitions cycle over")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    graphs, num_nodes = bm.build_mag_like(dev)
    etypes, ntypes = sorted(graphs), sorted(num_nodes)
    g = torch.Generator(device=dev).manual_seed(5)
    tables = {t: torch.rand((num_nodes[t], bm.F_IN), generator=g, device=dev) * 2 - 1 for t in ntypes}
    B, G = args.batch_size, args.call_group
    seeds = torch.randperm(num_nodes["paper"], generator=g, device=dev)[:args.groups * G * B]
    groups = list(bm.make_loader(bm.build_mag_like.graph_store, tables, seeds, B, G).call_groups())
    torch.manual_seed(0)
    model = [nn.HeteroConv({et: nn.TransformerConv((fin, fin), args.hidden, heads=args.heads, concat=False) for et in etypes}).to(dev)
             for fin in (bm.F_IN, args.hidden)]
    params = [p for m in model for p in m.parameters()]
    opt = torch.optim.SGD(params, lr=1e-4)
    data = [(grp.x_dict, [grp.layer_graph(0), grp.layer_graph(1)]) for grp in groups]
    gout = torch.randn((G * B, args.hidden), generator=g, device=dev) / (G * B)
    routes = {"grouped": grouped, "relation": relation_by_relation}
    with torch.no_grad():      # the two routes compute the same thing
        a, b = (fn(model, data[0][0], data[0][1], "relu") for fn in routes.values())
        parity = float((a - b).abs().max() / b.abs().max())
    turn = [0]

    def forward(fn):
        xs, lgs = data[turn[0] % len(data)]
        turn[0] += 1
        with torch.no_grad():
            fn(model, xs, lgs, "relu")

    def step(fn):
        xs, lgs = data[turn[0] % len(data)]
        turn[0] += 1
        opt.zero_grad(set_to_none=True)
        (fn(model, xs, lgs, "relu") * gout[:lgs[1].n_out["paper"]]).sum().backward()
        opt.step()

    res = {"forward": {k: [] for k in routes}, "train_step": {k: [] for k in routes}}
    for what, run, reps in (("forward", forward, args.reps), ("train_step", step, args.reps)):
        for name, fn in routes.items():                       # warm-up of both, then the routes interleaved rep by rep
            timed(lambda: run(fn), 0, args.warmup)
        for _ in range(reps):
            for name, fn in routes.items():
                res[what][name] += timed(lambda: run(fn), 1, 0)
    launches = nn.hetero_transformer_launches
    line = {"workload": "ogbn-mag-like hetero (bench_mag.build_mag_like), fan-out [25, 10], F_in %d, 2 x HeteroConv{TransformerConv(hidden %d, "
                        "heads %d, concat=False)}" % (bm.F_IN, args.hidden, args.heads),
            "batch_size": B, "call_group": G, "sampled_edges_per_group": int(sum(grp.num_edges for grp in groups) / len(groups)),
            "relative_difference_of_the_routes": parity, "hetero_transformer_launches": launches,
            "forward": {k: stats(v) for k, v in res["forward"].items()}, "train_step": {k: stats(v) for k, v in res["train_step"].items()}}
    for what in ("forward", "train_step"):
        line[what]["relation_over_grouped"] = round(line[what]["relation"]["median_ms"] / line[what]["grouped"]["median_ms"], 3)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
