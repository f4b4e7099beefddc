#!/usr/bin/env python
"""RowLinear (csrc/wg_row_linear.hip, ``wholegraph_amd.nn.linear_rows``) against the torch formulation it replaces — a gather of
the rows (converting, for a 16-bit table), ``F.linear``, relu, ``F.layer_norm`` / ``F.normalize``, the add, and their autograd
nodes — in ONE job: the two routes alternate, repeat by repeat, and the median of the repeats is reported (HIP events around each
call, device-synchronised).

Cases (n rows each):
    projection   bfloat16 table of 2 n rows read through an int64 id list, K = 128, N = 64, LayerNorm      (paper_norm(paper_lin(x)))
    skip term    float32 [2 n, 64] input, n distinct rows given, K = N = 64, no norm                       (lin1(x[rows]))
    tail         float32 [n, 64] input, K = N = 64, ReLU, L2 norm, add                                     (normalize(lin2(x).relu()) + x0)
forward alone (no_grad) and forward + backward (gradients of the weights and the norm's parameters; of ``x`` and ``add`` too in the
skip term and the tail).

Algorithmic bytes per row of the FORWARD (what each route has to move through HBM at least; weights are cache-resident):
    kernel   index + input row + out (+ add)
    torch    gather: index + input row + [n, K] float32 copy written;  linear: copy read + y written;  relu: y read + written;
             norm: y read + z written;  add: z and add read + out written
"of 8 TB/s" is the kernel route's forward bytes over its measured forward time over the HBM peak.

    python tools/bench_row_linear.py [--rows 1000000] [--repeats 25] [--out profiles/row_linear/bench_row_linear.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cugraph-gnn_amd")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from wholegraph_amd import nn  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def make_case(name, n, dev):
    """``(x, rows, params, kwargs, go, bytes)``: ``params`` = the leaves that take a gradient; ``kwargs`` of ``linear_rows``."""
    g = torch.Generator(device=dev).manual_seed(0)
    mk = lambda *s: torch.randn(s, generator=g, device=dev)      # noqa: E731
    if name == "projection":
        K, N = 128, 64
        table = mk(2 * n, K).to(torch.bfloat16)
        x, rows = nn.LazyRows(table, torch.randint(0, 2 * n, (n,), generator=g, device=dev)), None
        w, b, gamma, beta = mk(N, K) / K ** 0.5, mk(N), mk(N), mk(N)
        kw, leaves, add = dict(norm="layer", norm_weight=gamma, norm_bias=beta), [w, b, gamma, beta], None
        kernel_bytes = 8 + 2 * K + 4 * N
        torch_bytes = (8 + 2 * K + 4 * K) + (4 * K + 4 * N) + (4 * N + 4 * N)
    elif name == "skip term":
        K = N = 64
        x, rows = mk(2 * n, K).requires_grad_(True), torch.randperm(2 * n, generator=g, device=dev)[:n]
        w, b, add = mk(N, K) / K ** 0.5, mk(N), None
        kw, leaves = dict(), [x, w, b]
        kernel_bytes = 8 + 4 * K + 4 * N
        torch_bytes = (8 + 4 * K + 4 * K) + (4 * K + 4 * N)
    else:
        K = N = 64
        x, rows, add = mk(n, K).requires_grad_(True), None, mk(n, N).requires_grad_(True)
        w, b = mk(N, K) / K ** 0.5, mk(N)
        kw, leaves = dict(relu=True, norm="l2", add=add), [x, w, b, add]
        kernel_bytes = 4 * K + 4 * N + 4 * N
        torch_bytes = (4 * K + 4 * N) + 8 * N + 8 * N + 12 * N
    for t in (w, b) + tuple(v for v in kw.values() if torch.is_tensor(v)):
        t.requires_grad_(True)
    return x, rows, w, b, kw, leaves, mk(n, N), kernel_bytes, torch_bytes


def torch_formulation(x, rows, w, b, kw):
    xr = x.materialize() if isinstance(x, nn.LazyRows) else x
    if rows is not None:
        xr = xr[rows]
    y = F.linear(xr, w, b)
    if kw.get("relu"):
        y = y.relu()
    if kw.get("norm") == "layer":
        y = F.layer_norm(y, (y.shape[1],), kw["norm_weight"], kw["norm_bias"], 1e-5)
    elif kw.get("norm") == "l2":
        y = F.normalize(y, p=2, dim=-1)
    return y if kw.get("add") is None else y + kw["add"]


def bench_case(name, n, repeats, warmup):
    x, rows, w, b, kw, leaves, go, kernel_bytes, torch_bytes = make_case(name, n, "cuda")

    def call(route):
        if route == "kernel":
            return nn.linear_rows(x, w, b, rows=rows, **kw)
        if isinstance(x, nn.LazyRows):
            x._rows = None                                      # (every call gathers, as every mini-batch does)
        return torch_formulation(x, rows, w, b, kw)

    def fwd(route):
        with torch.no_grad():
            return call(route)

    def fwd_bwd(route):
        call(route).backward(go)
        for leaf in leaves:
            leaf.grad = None

    before = nn.row_linear_launches
    times = {(r, p): [] for r in ("kernel", "torch") for p in ("fwd", "fwd_bwd")}
    for k in range(warmup + repeats):
        for route in ("kernel", "torch"):                       # interleaved: both routes see the same machine state
            for what, fn in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                ms = timed(lambda: fn(route))
                if k >= warmup:
                    times[(route, what)].append(ms)
    assert nn.row_linear_launches - before == 2 * (warmup + repeats), "the kernel route did not launch once per call"
    res = {"case": name, "rows": n, "repeats": repeats, "kernel_fwd_bytes_per_row": kernel_bytes, "torch_fwd_bytes_per_row": torch_bytes}
    for (route, what), v in times.items():
        res["%s_%s_ms" % (route, what)] = round(statistics.median(v), 4)
        res["%s_%s_min_ms" % (route, what)] = round(min(v), 4)
    res["kernel_fwd_of_peak"] = round(n * kernel_bytes / (res["kernel_fwd_ms"] * 1e-3) / HBM_PEAK, 3)
    res["speedup_fwd"] = round(res["torch_fwd_ms"] / res["kernel_fwd_ms"], 2)
    res["speedup_fwd_bwd"] = round(res["torch_fwd_bwd_ms"] / res["kernel_fwd_bwd_ms"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X (there is no CPU fallback)"
    assert args.repeats >= 20 or args.rows < 100_000, "report the median of at least 20 repeats"
    results = []
    print("| case | bytes/row kernel, torch | kernel fwd ms (of 8 TB/s) | torch fwd ms | kernel fwd+bwd ms | torch fwd+bwd ms | speed-up fwd, fwd+bwd |")
    print("|---|---|---|---|---|---|---|")
    for name in ("projection", "skip term", "tail"):
        r = bench_case(name, args.rows, args.repeats, args.warmup)
        results.append(r)
        print("| %s | %d, %d | %.3f (%.2f) | %.3f | %.3f | %.3f | %.2fx, %.2fx |" % (
            name, r["kernel_fwd_bytes_per_row"], r["torch_fwd_bytes_per_row"], r["kernel_fwd_ms"], r["kernel_fwd_of_peak"],
            r["torch_fwd_ms"], r["kernel_fwd_bwd_ms"], r["torch_fwd_bwd_ms"], r["speedup_fwd"], r["speedup_fwd_bwd"]), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return results


if __name__ == "__main__":
    main()
