#!/usr/bin/env python
"""The three GATv2 kernels (csrc/wg_gatv2.hip) on their own at the deep-hop shape of a products-like call group — 16 mini-batches
of 1024 seeds, fan-out [25, 10]: 409 600 destination rows of 10 sampled edges and a self loop each over 2 M input rows, H = 4,
C = 64 — timed with HIP events, each against its algorithmic bytes:

    forward              E' (4 HC + 4) + n_dst 8 HC                       (+ 8 E' H + n_dst 4 HC when training: logits, agg)
    backward, dst-major  E' (4 HC + 4 + 8 H) + n_dst 16 HC + (n_dst / 16) 4 HC
    backward, src-major  E' (8 HC + 8 + 8 H) + n_src 12 HC

(E' counts the self loops).  Writes <out-dir>/bench_gatv2.json and prints it; with --trace it then runs itself under
`rocprofv3 --kernel-trace --stats` in a fresh process and puts the per-kernel table beside it (bench_gatv2_kernel_stats.csv).

    python tools/bench_gatv2.py [--iters 20] [--out-dir profiles/gatv2] [--trace]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dst-rows", type=int, default=16 * 1024 * 25)
    ap.add_argument("--src-rows", type=int, default=2_000_000)
    ap.add_argument("--fanout", type=int, default=10)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "gatv2"))
    ap.add_argument("--trace", action="store_true", help="also run under rocprofv3 --kernel-trace --stats (a fresh process)")
    ap.add_argument("--no-write", action="store_true", help="print only (the traced child)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from wholegraph_amd import nn
    dev = torch.device("cuda")
    n, n_src, H, C = args.dst_rows, args.src_rows, args.heads, args.channels
    HC = H * C
    g = torch.Generator(device=dev).manual_seed(0)
    rp = (torch.arange(n + 1, device=dev) * args.fanout).to(torch.int32)
    col = torch.randint(0, n_src, (n * args.fanout,), generator=g, device=dev, dtype=torch.int32)
    self_rows = torch.randperm(n_src, generator=g, device=dev)[:n].contiguous()
    hop = nn._gatv2_hop(nn.HopGraph(rp, col, self_rows), True)
    E = int(hop.col.shape[0])
    XL = torch.randn((n_src, HC), generator=g, device=dev)
    XR = torch.randn((n, HC), generator=g, device=dev)
    att = torch.randn((1, H, C), generator=g, device=dev) * (3.0 / C ** 0.5)
    bias = torch.zeros(HC, device=dev)
    G = torch.randn((n, HC), generator=g, device=dev)
    out = torch.empty((n, HC), device=dev)
    _, alpha, agg = nn.gatv2_attention(hop.row_ptr, hop.col, XL, XR, att, H, bias=bias, relu=True, out=out, need_alpha=True)
    dxr, de, _ = nn.gatv2_bwd_dst(hop.row_ptr, hop.col, XL, XR, att, H, alpha, G, agg)
    row_ptr_t, col_t, _, perm = hop.transposed(n_src, need_self=False, need_perm=True)
    gx = torch.zeros((n_src, HC), device=dev)
    t = {
        "forward": timed(lambda: nn.gatv2_attention(hop.row_ptr, hop.col, XL, XR, att, H, bias=bias, relu=True, out=out), args.iters),
        "forward_train": timed(lambda: nn.gatv2_attention(hop.row_ptr, hop.col, XL, XR, att, H, bias=bias, relu=True, out=out,
                                                          need_alpha=True), args.iters),
        "bwd_dst": timed(lambda: nn.gatv2_bwd_dst(hop.row_ptr, hop.col, XL, XR, att, H, alpha, G, agg, dxr=dxr), args.iters),
        "bwd_src": timed(lambda: nn.gatv2_bwd_src(row_ptr_t, col_t, perm, XL, XR, att, H, alpha, de, G, gx), args.iters),
    }
    fwd = E * (4 * HC + 4) + n * 8 * HC
    b = {"forward": fwd, "forward_train": fwd + 8 * E * H + n * 4 * HC,
         "bwd_dst": E * (4 * HC + 4 + 8 * H) + n * 16 * HC + (n // 16) * 4 * HC,
         "bwd_src": E * (8 * HC + 8 + 8 * H) + n_src * 12 * HC}
    res = {k: {"ms": round(t[k], 4), "bytes": b[k], "TB_per_s": round(b[k] / (t[k] * 1e-3) / 1e12, 3),
               "fraction_of_8TBps": round(b[k] / (t[k] * 1e-3) / HBM_PEAK, 3)} for k in t}
    line = json.dumps({"metric": "gatv2_forward_ms", "value": res["forward"]["ms"], "unit": "ms",
                       "shape": {"dst_rows": n, "src_rows": n_src, "entries_with_self_loops": E, "H": H, "C": C,
                                 "max_transposed_degree": int((row_ptr_t[1:] - row_ptr_t[:-1]).max())}, "kernels": res})
    print(line)
    if args.no_write:
        return
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "bench_gatv2.json"), "w") as f:
        f.write(line + "\n")
    if args.trace:
        with tempfile.TemporaryDirectory() as tmp:
            subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "gatv2", "--",
                                   sys.executable, os.path.abspath(__file__), "--iters", "3", "--no-write", "--dst-rows", str(n),
                                   "--src-rows", str(n_src), "--fanout", str(args.fanout), "--heads", str(H), "--channels", str(C)],
                                  stdout=subprocess.DEVNULL)
            found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            assert found, "rocprofv3 wrote no kernel_stats.csv"
            shutil.copy(found[0], os.path.join(args.out_dir, "bench_gatv2_kernel_stats.csv"))


if __name__ == "__main__":
    main()
