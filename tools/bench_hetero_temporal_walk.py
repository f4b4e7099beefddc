#!/usr/bin/env python
"""`HeteroPygWalk.run` alone on the graph of examples/temporal_hetero_link_call_groups.py: the temporal walk, uniform and biased,
beside the non-temporal biased walk over the same ragged seed lists of both node types.  HIP events around `run`, warm-up runs
first, then `--rounds` alternating rounds of `--iters` runs each; prints per configuration the median of every round (ms), the
edges one run samples and its live (hop, edge type) calls, as JSON.

    python tools/bench_hetero_temporal_walk.py [--users 6040] [--items 3706] [--avg-degree 166] [--fanout 5 5 5] [--group 8]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cugraph-gnn_amd"), os.path.join(ROOT, "examples")]

import torch  # noqa: E402

import temporal_hetero_link_call_groups as ex  # noqa: E402
from cugraph_pyg_amd.data import FeatureStore, GraphStore  # noqa: E402
from cugraph_pyg_amd.sampler.sampler import _as_i64, hop_seed  # noqa: E402
from wholegraph_amd.fused import HeteroPygWalk  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=6040)
    ap.add_argument("--items", type=int, default=3706)
    ap.add_argument("--avg-degree", type=int, default=166)
    ap.add_argument("--fanout", type=int, nargs="+", default=[5, 5, 5])
    ap.add_argument("--group", type=int, default=8, help="mini-batches per walk")
    ap.add_argument("--seeds", type=int, default=768, help="seeds per mini-batch and node type")
    ap.add_argument("--seed-time", type=int, default=500, help="edge times are uniform in [0, 1000)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    U, I, G, B = args.users, args.items, args.group, args.seeds
    E = U * args.avg_degree
    rates, when, _, _ = ex.planted_ratings(U, I, E, 20, 1000, dev, g)
    gs, fs = GraphStore(), FeatureStore()
    gs[ex.RATES, "coo", False, (U, I)] = rates
    gs[ex.REV_RATES, "coo", False, (I, U)] = rates.flip(0)
    weight = torch.rand(E, generator=g, device=dev) + 0.05
    for et in (ex.RATES, ex.REV_RATES):
        fs[et, "time", None] = when
        fs[et, "w", None] = weight
    gs._set_time_attr((fs, "time"))
    gs._set_weight_attr((fs, "w"))
    graphs = gs._hetero_graphs
    fan = {et: list(args.fanout) for et in graphs}
    counts = {"user": U, "item": I}
    ids = {"user": torch.randint(0, U, (G * B,), generator=g, device=dev), "item": torch.randint(0, I, (G * B,), generator=g, device=dev)}
    seg = (torch.arange(G + 1, dtype=torch.int32, device=dev) * B).contiguous()
    batch = torch.arange(G, dtype=torch.int32, device=dev).repeat_interleave(B).contiguous()
    times = torch.full((G * B,), args.seed_time, dtype=torch.int64, device=dev)
    rs = torch.tensor([[_as_i64(hop_seed(100 + j, k)) for j in range(G)] for k in range(len(args.fanout) * len(graphs))],
                      dtype=torch.int64)

    def walk(biased, comparison):
        return HeteroPygWalk(graphs, B, fan, G, biased=biased, num_nodes=counts, pad_unique=False, temporal_comparison=comparison)

    walks = {"temporal uniform": walk(False, "monotonically_decreasing"), "temporal biased": walk(True, "monotonically_decreasing"),
             "non-temporal biased": walk(True, None)}

    def run(w):
        extra = (times,) if w.comparison else ()
        return w.run(None, None, rs, seed_lists={t: (ids[t], seg, batch) + extra for t in ids})

    out = {}
    for name, w in walks.items():
        for _ in range(3):
            rec = run(w)
        torch.cuda.synchronize()
        live = [c for c in rec["calls"] if c is not None]
        out[name] = dict(edges_per_run=sum(int(c["counts"][0]) for c in live), calls=len(live), median_ms_per_round=[])
    for _ in range(args.rounds):
        for name, w in walks.items():
            ms = []
            for _ in range(args.iters):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run(w)
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            out[name]["median_ms_per_round"].append(round(statistics.median(ms), 4))
    print(json.dumps(out, indent=1))
    return out


if __name__ == "__main__":
    main()
