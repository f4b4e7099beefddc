"""The one-kernel SAGE layer hands its 64-row tiles out by ticket: the first tile of a workgroup is its block index, every
later one comes from a device counter that the launch's last workgroup rewinds.  A row's tile — and with it every bit of its
output — does not depend on which workgroup runs the tile, so any two schedules must agree bit for bit; the counter slot must
be back at zero for whatever launch uses it next (same stream, another stream, a graph replay).

Row counts (C = compute units): one partial tile; 64 C (no ticket ever names a tile); 64 C + 1 (one does); 64 (2 C + 3) + 17
(several rounds and a partial last tile).  Layers: F = 100 -> 256 (compile-time shape, whole tiles in LDS) with and without
an int32 node list, F = 256 -> 47 (half tiles, one multiplying wave, runtime shape), ReLU on and off.  Every row count is a
prefix of ONE graph per layer, so one float64 reference per layer serves them all."""
import functools

import numpy as np
import pytest

from graphgen import powerlaw_csr
from layer_graphs import empty_hop_graph

pytestmark = pytest.mark.gpu

LAYERS = {"100x256_ids": (100, 256, True), "100x256": (100, 256, False), "256x47": (256, 47, False)}


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _row_counts():
    C = _cus()
    return {"partial": 41, "64C": 64 * C, "64C+1": 64 * C + 1, "rounds": 64 * (2 * C + 3) + 17}


@functools.lru_cache(maxsize=None)
def _case(layer):
    """Inputs on the device and the float64 results (before the activation) + error scale of ALL rows; never modified."""
    import torch
    F, N, with_ids = LAYERS[layer]
    n_max = max(_row_counts().values())
    rp, col = powerlaw_csr(n_max, 8, seed=F + N, col_dtype=np.int32, max_deg=60)   # rows past both neighbour windows too
    rng = np.random.default_rng(7 * F + N)
    n_src, V = n_max, 3 * n_max
    cu = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    table = cu(rng.standard_normal((V if with_ids else n_src, F)).astype(np.float32))
    ids = cu(rng.permutation(V)[:n_src].astype(np.int32)) if with_ids else None
    self_rows = cu(rng.integers(0, n_src, n_max).astype(np.int64))
    w_t = cu((rng.standard_normal((2 * F, N)) * 0.2).astype(np.float32))
    bias = cu(rng.standard_normal(N).astype(np.float32))
    rp, col = cu(rp.astype(np.int32)), cu(col)
    # float64 formulation: mean over the CSR row, [mean | self] @ w_t + bias
    x64 = (table[ids.long()] if with_ids else table).double()
    deg = (rp[1:] - rp[:-1]).long()
    owner = torch.repeat_interleave(torch.arange(n_max, device="cuda"), deg)
    agg = torch.zeros((n_max, F), dtype=torch.float64, device="cuda").index_add_(0, owner, x64[col.long()])
    agg /= deg.clamp(min=1).unsqueeze(1)
    cat = torch.cat([agg, x64[self_rows]], 1)
    ref = cat @ w_t.double() + bias.double()
    scale = cat.abs() @ w_t.double().abs() + bias.double().abs()
    return dict(rp=rp, col=col, table=table, ids=ids, self_rows=self_rows, w_t=w_t, bias=bias, ref=ref, scale=scale, agg=agg)


def _run(c, lo, hi, relu, **kw):
    """The layer over rows [lo, hi) of the case as ONE launch.  (A launch's row_ptr starts at 0 — the kernel reads row_ptr[0]
    as a stand-in neighbour for the slots past a row's degree — so the slice is rebased and `col` enters at its first edge.)"""
    from wholegraph_amd import nn
    e0 = int(c["rp"][lo]) if lo else 0      # (no read-back for a launch from row 0: it may be under graph capture)
    rp = (c["rp"][lo:hi + 1] - e0).contiguous() if lo else c["rp"][:hi + 1]
    return nn.sage_layer_fused_forward(rp, c["col"][e0:], c["table"], c["self_rows"][lo:hi].contiguous(),
                                       c["w_t"], c["bias"], relu=relu, mean=True, src_ids=c["ids"], precision="bf16x3", **kw)


@functools.lru_cache(maxsize=None)
def _eager(layer, n, relu):
    return _run(_case(layer), 0, n, relu)


def _check_fp64(got, c, n, relu):
    """tests/test_gpu_aggregate.py's bounds for this kernel: |err| <= 1e-5 * sum |a||b| + 1e-6 everywhere, and 1e-5 relative
    wherever the result is not a cancellation (|ref| >= 0.1 * scale)."""
    import torch
    ref, scale = c["ref"][:n], c["scale"][:n]
    if relu:
        ref = ref.clamp(min=0)
    err = (got.double() - ref).abs()
    big = ref.abs() >= 0.1 * scale
    print("max err %.3e, max err / bound %.3f, max rel %.3e" % (float(err.max()), float((err / (1e-5 * scale + 1e-6)).max()),
                                                                  float((err[big] / ref.abs()[big]).max())))
    assert torch.all(err <= 1e-5 * scale + 1e-6), float(err.max())
    assert bool(big.any()) and float((err[big] / ref.abs()[big]).max()) <= 1e-5


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("rows", ["partial", "64C", "64C+1", "rounds"])
@pytest.mark.parametrize("layer", list(LAYERS))
def test_schedule_independence_bit_for_bit(hiplib, layer, rows, relu):
    import torch
    c, n = _case(layer), _row_counts()[rows]
    whole = _eager(layer, n, relu)
    _check_fp64(whole, c, n, relu)
    assert torch.equal(_run(c, 0, n, relu), whole), "the same launch twice"
    # the same rows as two launches: [0, 64 m) and [64 m, n) — every row keeps its tile, the tiles change workgroups
    m = (n // 64) // 3
    parts = [_run(c, 0, 64 * m, relu), _run(c, 64 * m, n, relu)]
    assert parts[0].shape[0] == 64 * m
    assert torch.equal(torch.cat(parts), whole), "split launch"
    # a prefix of a longer launch is the same rows in the same tiles
    assert torch.equal(_eager(layer, max(_row_counts().values()), relu)[:n], whole)


def test_training_entry_keeps_the_bits_and_the_aggregate(hiplib):
    import torch
    from wholegraph_amd import nn
    c, n = _case("100x256"), _row_counts()["rounds"]
    assert nn.sage_layer_train_supported(100, 256)
    agg = torch.empty((n, 100), device="cuda")
    out = _run(c, 0, n, True, agg_out=agg)
    assert torch.equal(out, _eager("100x256", n, True))
    ref = c["agg"][:n]
    assert torch.all((agg.double() - ref).abs() <= 1e-5 * ref.abs() + 1e-6)


def test_counter_slot_reuse_one_stream_and_two_streams(hiplib):
    import torch
    c1, c2, n = _case("100x256_ids"), _case("256x47"), _row_counts()["rounds"]
    want1, want2 = _eager("100x256_ids", n, True), _eager("256x47", n, False)
    for _ in range(3):      # back to back on one stream: each launch finds the slot the one before left
        got1, got2 = _run(c1, 0, n, True), _run(c2, 0, n, False)
        assert torch.equal(got1, want1) and torch.equal(got2, want2)
    # two streams at once, three launches each: they must not share a slot
    streams, got = [torch.cuda.Stream(), torch.cuda.Stream()], [[], []]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    for _ in range(3):
        for i, (s, c, relu) in enumerate(zip(streams, (c1, c2), (True, False))):
            with torch.cuda.stream(s):
                got[i].append(_run(c, 0, n, relu))
    for s in streams:
        torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert all(torch.equal(g, want1) for g in got[0]) and all(torch.equal(g, want2) for g in got[1])


def test_graph_replay_starts_from_a_rewound_slot(hiplib):
    import torch
    c1, c2, n = _case("100x256"), _case("256x47"), _row_counts()["rounds"]
    want1, want2 = _eager("100x256", n, True), _eager("256x47", n, True)
    out1 = torch.zeros((n, 256), device="cuda")
    pad2 = torch.zeros((n, 64), device="cuda")       # the 47-wide head runs at 64 columns: a view of the padded buffer
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                    # (warm-up on the side stream, as torch asks before a capture)
        _run(c1, 0, n, True, out=out1), _run(c2, 0, n, True, out=pad2[:, :47])
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _run(c1, 0, n, True, out=out1)
        _run(c2, 0, n, True, out=pad2[:, :47])
    for _ in range(3):
        out1.zero_(), pad2.zero_()
        g.replay()
        # an eager launch next to the replays (own slot: the capture's belongs to the graph)
        assert torch.equal(_run(c1, 0, n, True), want1)
        assert torch.equal(out1, want1) and torch.equal(pad2[:, :47], want2)


def test_edge_less_hop_and_no_rows(hiplib):
    import torch
    from wholegraph_amd import nn
    F, N, n_src = 100, 256, 300
    lg, _, _ = empty_hop_graph(n_src, seed=11)
    g = torch.Generator(device="cuda").manual_seed(12)
    x = torch.randn((n_src, F), generator=g, device="cuda")
    w_t = torch.randn((2 * F, N), generator=g, device="cuda") * 0.2
    bias = torch.randn(N, generator=g, device="cuda")
    hop = lg.hops[1]                                    # 40 destinations, no edge: out = x[self] @ W_r^T + b
    got = nn.sage_layer_fused_forward(hop.row_ptr, hop.col, x, hop.self_rows, w_t, bias, relu=False, precision="bf16x3")
    cat = torch.cat([torch.zeros((40, F), dtype=torch.float64, device="cuda"), x[hop.self_rows].double()], 1)
    ref, scale = cat @ w_t.double() + bias.double(), cat.abs() @ w_t.double().abs() + bias.double().abs()
    assert torch.all((got.double() - ref).abs() <= 1e-5 * scale + 1e-6)
    none = nn.sage_layer_fused_forward(torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"),
                                       x, torch.zeros(0, dtype=torch.int64, device="cuda"), w_t, bias, precision="bf16x3")
    assert none.shape == (0, N)
    # and the launches after them still find their slot at zero
    assert torch.equal(nn.sage_layer_fused_forward(hop.row_ptr, hop.col, x, hop.self_rows, w_t, bias, relu=False, precision="bf16x3"), got)
