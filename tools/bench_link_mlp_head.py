#!/usr/bin/env python
"""The MLP edge decoder (`nn.EdgeDecoder` / `nn.link_mlp_bce_with_logits`, csrc/wg_link_mlp.hip) against its torch formulation,
on the pairs of tools/bench_link_head.py's products-shaped link call group (P = 188 * 2048 pairs over the group's seed rows, one
table on both sides), C = H = 64 and C = H = 256, timed with HIP events after 3 warm-up calls: the BCE forward alone (no grad
mode) and forward + backward (gradients of the table and the four parameters), kernel route and torch ops in the same process.
Byte model of the forward, printed beside the times:
    rows + scores:  P (8 C + 16 + 4)  +  4 P      (two rows, two int64 indices and a label per pair; the coefficient)
    W1 from L2:     ceil(P / 16) * H * 2 C * 4    (every 16-pair tile reads all of W1 again)
Prints one JSON line.

    python tools/bench_link_mlp_head.py [--iters 20] [--group 188]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cugraph-gnn_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_link_head import products_link_group, timed  # noqa: E402


def head_timings(grp, C, iters, gen):
    from wholegraph_amd import nn
    eli, label = grp.edge_label_index, (grp.edge_label > 0).float()
    P, dev = eli.shape[1], eli.device
    h = torch.randn((grp.num_seeds, C), generator=gen, device=dev, requires_grad=True)
    torch.manual_seed(C)
    dec = nn.EdgeDecoder(C).to(dev)
    leaves = [h] + list(dec.parameters())

    def torch_loss():
        z = torch.cat([h[eli[0]], h[eli[1]]], dim=-1)
        return F.binary_cross_entropy_with_logits(dec.lin2(dec.lin1(z).relu()).view(-1), label)

    def kernel_fwd():
        with torch.no_grad():
            return dec.loss(h, h, eli, label)

    def torch_fwd():
        with torch.no_grad():
            return torch_loss()

    def both(loss):
        def run():
            for t in leaves:
                t.grad = None
            loss().backward()
        return run

    assert type(dec.loss(h, h, eli, label).grad_fn).__name__ == "_PairMlpBackward"       # (the kernel route, not its fallback)
    t = {"kernel_fwd_ms": timed(kernel_fwd, iters), "torch_fwd_ms": timed(torch_fwd, iters),
         "kernel_fwd_bwd_ms": timed(both(lambda: dec.loss(h, h, eli, label)), iters),
         "torch_fwd_bwd_ms": timed(both(torch_loss), iters)}
    out = {k: round(v, 4) for k, v in t.items()}
    rows_gb = (P * (8 * C + 16 + 4) + 4 * P) / 1e9
    w1_gb = ((P + 15) // 16) * C * 2 * C * 4 / 1e9
    out.update(C=C, H=C, pairs=P, seed_rows=grp.num_seeds, fwd_rows_and_scores_GB=round(rows_gb, 4), fwd_w1_from_l2_GB=round(w1_gb, 4),
               loss_kernel=round(float(kernel_fwd()), 6), loss_torch=round(float(torch_fwd()), 6))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", type=int, default=188, help="mini-batches per call group")
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    grp, loader, g = products_link_group(args.group)
    heads = [head_timings(grp, C, args.iters, g) for C in (64, 256)]
    print(json.dumps({"metric": "link_mlp_head", "group": args.group, "heads": heads}))


if __name__ == "__main__":
    main()
