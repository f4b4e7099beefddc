#!/usr/bin/env python
"""One Linear per node type over ogbn-mag-like row counts, two routes in one process:

  * grouped  — ``nn.HeteroDictLinear``: ONE ``wgamd_grouped_linear_f32`` launch for all types (csrc/wg_grouped_linear.hip), and in
    the backward one dX launch, one weight-gradient launch and one reduce launch;
  * per_type — what the package offered before: one ``nn.linear_rows`` call per type with the same parameters (one
    ``wgamd_row_linear_f32`` launch each; per type a library GEMM for dX and a ``gcn_wgrad`` pipeline in the backward).

Measured: the forward (no autograd) and forward + backward (inputs, weights and biases take gradients).  Every shape and route is
warmed up; a timing is a host clock around a window of repetitions that ends in a device synchronise and lasts at least
``--window`` seconds; the routes alternate window by window, ``--rounds`` times.  Before the clock starts the two routes' outputs
are compared at the timed size: ``|a - b| <= 1e-5 x sum|terms|`` element-wise, the bound of the tests.
Prints one JSON line per shape with median / min / max per route.

    python tools/bench_hetero_linear.py [--rows 600000,300000,50000,8000] [--shapes 128x64,256x256] [--rounds 3] [--window 0.5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cugraph-gnn_amd")]

import torch  # noqa: E402

from wholegraph_amd import nn  # noqa: E402

TYPES = ("paper", "author", "institution", "field_of_study")


def per_type(mod, xs, relu):
    return {t: nn.linear_rows(x, mod.lins[t].weight, mod.lins[t].bias, relu=relu) for t, x in xs.items()}


def grouped(mod, xs, relu):
    return mod(xs, relu=relu)


def window(fn, seconds):
    """Seconds per call of ``fn`` over a synchronised window of at least ``seconds`` (repetitions doubled until it is)."""
    reps = 1
    while True:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / reps
        reps = max(reps * 2, int(reps * seconds / max(dt, 1e-6)) + 1)


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(1e3 * ts[len(ts) // 2], 4), "min_ms": round(1e3 * ts[0], 4), "max_ms": round(1e3 * ts[-1], 4),
            "windows": len(ts)}


def bytes_and_flops(rows, K, N):
    """What one forward launch has to move and multiply: X once, W once per 64-row tile and column block, out once."""
    n = sum(rows)
    tiles = sum((r + 63) // 64 for r in rows)
    return {"flops": 2 * n * K * N, "hbm_bytes": 4 * (n * K + n * N + len(rows) * (K * N + N)), "weight_panel_bytes": 4 * tiles * K * N}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="600000,300000,50000,8000")
    ap.add_argument("--shapes", default="128x64,256x256")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--no-relu", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    rows = [int(r) for r in args.rows.split(",")]
    assert len(rows) <= len(TYPES) and args.rounds >= 2
    relu = not args.no_relu
    routes = {"grouped": grouped, "per_type": per_type}
    for shape in args.shapes.split(","):
        K, N = (int(v) for v in shape.split("x"))
        torch.manual_seed(0)
        mod = nn.HeteroDictLinear(K, N, types=TYPES[:len(rows)]).cuda()
        xs = {t: torch.randn(r, K, device="cuda").requires_grad_(True) for t, r in zip(TYPES, rows)}
        gos = [torch.randn(r, N, device="cuda") / r for r in rows]
        leaves = list(xs.values()) + list(mod.parameters())

        def forward(fn):
            with torch.no_grad():
                fn(mod, xs, relu)

        def step(fn):
            for p in leaves:
                p.grad = None
            torch.autograd.backward(list(fn(mod, xs, relu).values()), gos)

        # parity at the timed size, forward and every gradient
        got = {}
        for name, fn in routes.items():
            step(fn)
            with torch.no_grad():
                got[name] = [v.clone() for v in fn(mod, xs, relu).values()] + [p.grad.clone() for p in leaves]
        assert mod.route == "kernel"
        with torch.no_grad():
            worst = 0.0
            for t, a, b in zip(xs, got["grouped"], got["per_type"]):
                terms = xs[t].abs() @ mod.lins[t].weight.abs().t() + mod.lins[t].bias.abs()
                worst = max(worst, float(((a - b).abs() / (1e-5 * terms)).max()))
            assert worst <= 1.0, "the routes' outputs differ by %g of the bound" % worst
            grad_diff = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(got["grouped"][len(rows):],
                                                                                                     got["per_type"][len(rows):]))
        res = {"forward": {k: [] for k in routes}, "forward_backward": {k: [] for k in routes}}
        for what, run in (("forward", forward), ("forward_backward", step)):
            for fn in routes.values():                      # warm-up of both routes at this shape
                for _ in range(3):
                    run(fn)
            for _ in range(args.rounds):                    # the routes alternate window by window
                for name, fn in routes.items():
                    res[what][name].append(window(lambda: run(fn), args.window))
        line = {"workload": "one Linear per node type, rows %s, K %d, N %d, relu %s, float32" % (rows, K, N, relu),
                "forward_difference_over_bound": round(worst, 4), "largest_relative_gradient_difference": grad_diff,
                "per_forward_launch": bytes_and_flops(rows, K, N)}
        for what in res:
            line[what] = {k: stats(v) for k, v in res[what].items()}
            line[what]["per_type_over_grouped"] = round(line[what]["per_type"]["median_ms"] / line[what]["grouped"]["median_ms"], 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
