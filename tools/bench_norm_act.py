#!/usr/bin/env python
"""NormDropoutAct (csrc/wg_norm_act.hip, ``wholegraph_amd.nn.norm_dropout_act``) against the chain of torch ops it replaces —
add, ``layer_norm``, ``dropout`` (which writes a mask), ``relu`` and their autograd nodes, per node type — in ONE job: the two
routes alternate, repeat by repeat, and the median of the repeats is reported (HIP events around each call).

Shapes: [1.6 M, 64], [1.6 M, 256] and a four-type dict of [0.4 M, 128] each; every shape with and without residual; training
mode at p = 0.5; forward alone and forward + backward (gradients of x, residual, weight and bias).

Algorithmic bytes per row: forward ``(2 or 3) * 4 C + 8`` (x, residual, out, the two row statistics); backward ``(3 or 4) * 4 C``
(x, residual, grad_out, grad_in); "of 8 TB/s" is those bytes over the measured time over the HBM peak — for forward + backward
the bytes of both passes over the time of both.

    python tools/bench_norm_act.py [--repeats 25] [--p 0.5] [--out profiles/norm_act/bench_norm_act.json]
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
P = 0.5          # --p: the dropout probability (0: the kernels draw no mask, the torch chain's dropout is the identity)


def torch_chain(xs, ws, bs, rs):
    """What a model does per node type without the fused block."""
    out = {}
    for t, x in xs.items():
        z = x if rs is None else x + rs[t]
        z = F.layer_norm(z, (z.shape[1],), ws[t], bs[t], 1e-5)
        out[t] = torch.relu(F.dropout(z, P, True))
    return out


def kernel_block(xs, ws, bs, rs, seed):
    return nn.norm_dropout_act(xs, ws, bs, residual=rs, p=P, training=True, seed=seed)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bench_shape(name, shapes, with_res, repeats, warmup):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    mk = lambda n, c: torch.randn((n, c), generator=g, device=dev)      # noqa: E731
    xs = {t: mk(n, c).requires_grad_(True) for t, (n, c) in shapes.items()}
    rs = {t: mk(n, c).requires_grad_(True) for t, (n, c) in shapes.items()} if with_res else None
    ws = {t: torch.ones(c, device=dev, requires_grad=True) for t, (n, c) in shapes.items()}
    bs = {t: torch.zeros(c, device=dev, requires_grad=True) for t, (n, c) in shapes.items()}
    gs = {t: mk(n, c) for t, (n, c) in shapes.items()}
    leaves = list(xs.values()) + list(ws.values()) + list(bs.values()) + (list(rs.values()) if rs else [])

    def fwd(route, k):
        with torch.no_grad():
            return kernel_block(xs, ws, bs, rs, k) if route == "kernel" else torch_chain(xs, ws, bs, rs)

    def fwd_bwd(route, k):
        out = kernel_block(xs, ws, bs, rs, k) if route == "kernel" else torch_chain(xs, ws, bs, rs)
        torch.autograd.backward([out[t] for t in out], [gs[t] for t in out])
        for leaf in leaves:
            leaf.grad = None

    before = nn.norm_act_launches
    times = {(r, p): [] for r in ("kernel", "torch") for p in ("fwd", "fwd_bwd")}
    for k in range(warmup + repeats):
        for route in ("kernel", "torch"):                       # interleaved: both routes see the same machine state
            for what, fn in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                ms = timed(lambda: fn(route, k))
                if k >= warmup:
                    times[(route, what)].append(ms)
    assert nn.norm_act_launches - before == 2 * (warmup + repeats), "the kernel route did not launch once per call"
    rows = sum(n for n, _ in shapes.values())
    nbuf = 3 if with_res else 2
    fwd_bytes = sum(n * (nbuf * 4 * c + 8) for n, c in shapes.values())
    bwd_bytes = sum(n * ((nbuf + 1) * 4 * c) for n, c in shapes.values())
    res = {"shape": name, "rows": rows, "residual": with_res, "p": P, "repeats": repeats,
           "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes}
    for (route, what), v in times.items():
        med = statistics.median(v)
        nbytes = fwd_bytes if what == "fwd" else fwd_bytes + bwd_bytes
        res["%s_%s_ms" % (route, what)] = round(med, 4)
        res["%s_%s_min_ms" % (route, what)] = round(min(v), 4)
        res["%s_%s_of_peak" % (route, what)] = round(nbytes / (med * 1e-3) / HBM_PEAK, 3)
    res["speedup_fwd"] = round(res["torch_fwd_ms"] / res["kernel_fwd_ms"], 2)
    res["speedup_fwd_bwd"] = round(res["torch_fwd_bwd_ms"] / res["kernel_fwd_bwd_ms"], 2)
    return res


def main():
    global P
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1_600_000, help="rows of the single-tensor shapes (the dict has a quarter per type)")
    ap.add_argument("--p", type=float, default=P, help="dropout probability (default 0.5)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    P = args.p
    assert torch.cuda.is_available(), "needs an MI355X (there is no CPU fallback)"
    assert args.repeats >= 20 or args.rows < 100_000, "report the median of at least 20 repeats"
    n = args.rows
    cases = [("[%d, 64]" % n, {"x": (n, 64)}), ("[%d, 256]" % n, {"x": (n, 256)}),
             ("4 x [%d, 128]" % (n // 4), {t: (n // 4, 128) for t in ("paper", "author", "institution", "field")})]
    results = []
    print("| shape | residual | kernel fwd ms (of 8 TB/s) | torch fwd ms | kernel fwd+bwd ms (of 8 TB/s) | torch fwd+bwd ms | speed-up fwd, fwd+bwd |")
    print("|---|---|---|---|---|---|---|")
    for name, shapes in cases:
        for with_res in (False, True):
            r = bench_shape(name, shapes, with_res, args.repeats, args.warmup)
            results.append(r)
            print("| %s | %s | %.3f (%.2f) | %.3f | %.3f (%.2f) | %.3f | %.2fx, %.2fx |" % (
                name, "yes" if with_res else "no", r["kernel_fwd_ms"], r["kernel_fwd_of_peak"], r["torch_fwd_ms"],
                r["kernel_fwd_bwd_ms"], r["kernel_fwd_bwd_of_peak"], r["torch_fwd_bwd_ms"], r["speedup_fwd"], r["speedup_fwd_bwd"]),
                flush=True)
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return results


if __name__ == "__main__":
    main()
