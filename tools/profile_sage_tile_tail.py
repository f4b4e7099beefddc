"""When do the workgroups of the one-kernel SAGE layer finish?  Layer-1 launch at the products shape (1.617 M rows, F = 100 ->
256, int32 node list, ~14.6 M edges), alone and next to a second stream that runs the call-group walk + `unique`, on a library
built with the per-workgroup clock of tools/tune/sage_wg_clock.py (WGAMD_LIBRARY_PATH).  Prints, over the launches, the
max-minus-median of the workgroups' END times — the tail a fixed tile count per workgroup leaves — and the launch's span."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cugraph-gnn_amd")]
import bench  # noqa: E402
from wholegraph_amd import _lib, fused, nn  # noqa: E402
from wholegraph_amd.tensor import unique_bounded_nosync  # noqa: E402

TICK_US = 0.01      # wall_clock64: 100 MHz


def stamps():
    buf = (ctypes.c_ulonglong * 2048)()
    rc = ctypes.CDLL(_lib.LIB_PATH).wgamd_dbg_wg_clock(buf)
    assert rc == 0, rc
    a = np.frombuffer(buf, dtype=np.uint64).reshape(2, 1024).astype(np.int64)
    live = a[1] > 0
    return a[0][live], a[1][live]


def describe(tag, recs):
    sp = np.array([r[0] for r in recs]); span = np.array([r[1] for r in recs]); late = np.array([r[2] for r in recs])
    p10 = np.array([r[3] for r in recs])
    print("%s: launches %d | END max-median us: median %.1f mean %.1f min %.1f max %.1f | END max-p10 median %.1f | span us: median %.1f mean %.1f min %.1f | "
          "BEGIN max-min median %.1f" % (tag, len(recs), np.median(sp), sp.mean(), sp.min(), sp.max(), np.median(p10), np.median(span), span.mean(),
                                         span.min(), np.median(late)), flush=True)


def one_record():
    b, e = stamps()
    t0 = b.min()
    return ((e.max() - np.median(e)) * TICK_US, (e.max() - t0) * TICK_US, (b.max() - t0) * TICK_US, (e.max() - np.percentile(e, 10)) * TICK_US, len(e))


def main():
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    F, N = int(os.environ.get("F", 100)), int(os.environ.get("N", 256))
    n_dst, n_src, V = int(os.environ.get("ND", 1_617_000)), int(os.environ.get("NS", 2_300_000)), 2_449_029
    deg = torch.randint(5, 14, (n_dst,), generator=g, device=dev)
    rp = torch.zeros(n_dst + 1, dtype=torch.int32, device=dev)
    rp[1:] = torch.cumsum(deg, 0)
    E = int(rp[-1])
    col = torch.randint(0, n_src, (E,), generator=g, device=dev, dtype=torch.int32)
    table = torch.rand((V, F), generator=g, device=dev)
    n_id = torch.randint(0, V, (n_src,), generator=g, device=dev).to(torch.int32)
    rows = torch.randint(0, n_src, (n_dst,), generator=g, device=dev)
    w_t = torch.rand((2 * F, N), generator=g, device=dev) - 0.5
    bias = torch.rand(N, generator=g, device=dev)
    out = torch.empty((n_dst, N), device=dev)
    layer = lambda: nn.sage_layer_fused_forward(rp, col, table, rows, w_t, bias, relu=True, src_ids=n_id, out=out)  # noqa: E731
    print("rows %d edges %d F %d N %d" % (n_dst, E, F, N), flush=True)
    for _ in range(5):
        layer()
    torch.cuda.synchronize()
    stamps()
    recs = []
    for _ in range(int(os.environ.get("ITERS", 30))):
        layer()
        recs.append(one_record())
    print("workgroups", recs[0][4])
    describe("alone", recs)
    # HIP-event time of 20 back-to-back launches
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(20):
        layer()
    e.record()
    torch.cuda.synchronize()
    print("alone, events: %.4f ms per launch" % (s.elapsed_time(e) / 20), flush=True)
    stamps()
    if os.environ.get("WALK", "1") != "1":
        return
    # the walk of bench.py's products call group on a second stream
    G = int(os.environ.get("G", 188))
    wv, we, _, _, fanout = bench.WORKLOADS["products"]
    bench.FANOUT = fanout
    row_ptr, gcol = bench.rmat_csr(wv, we, seed=0, device=torch.device("cuda:0"))
    gcol = gcol.to(torch.int64)
    walk = fused.NoSyncWalk(row_ptr, gcol, bench.BATCH, bench.FANOUT, gcol.dtype, G, pad_unique=False)
    seeds = torch.randint(0, row_ptr.numel() - 1, (G * bench.BATCH,), generator=torch.Generator(device=dev).manual_seed(3), device=dev, dtype=gcol.dtype)
    hops = len(fanout)
    rs = (torch.arange(G, device=dev, dtype=torch.int64).view(1, -1) * hops + torch.arange(hops, device=dev, dtype=torch.int64).view(-1, 1) + 62)

    def walk_once(i):
        res = walk.run(seeds, rs + i * 7)
        unique_bounded_nosync(res.unique[hops - 1], res.counts[hops - 1][1:2], row_ptr.numel() - 1)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for i in range(3):
            walk_once(i)
    torch.cuda.synchronize()
    recs = []
    for i in range(int(os.environ.get("ITERS", 30))):
        with torch.cuda.stream(side):
            walk_once(i)          # ~1 ms of ~30 launches: under way when the layer launch starts
            walk_once(i + 100)
        layer()
        torch.cuda.synchronize()
        recs.append(one_record())
    describe("beside the walk", recs)


if __name__ == "__main__":
    main()
