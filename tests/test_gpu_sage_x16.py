"""The one-kernel SAGE layer over a float16 / bfloat16 feature table (``wgamd_sage_layer_fused_bf16x3_x``): the kernel loads the
16-bit rows and converts them to float32 exactly, so every output bit is that of the float32 route over ``table.float()``.

* ``nn.sage_layer_fused_forward`` with a 16-bit ``x`` read through int32 / int64 ids: ``torch.equal`` to the same call on
  ``table16.float()``, and within tests/test_gpu_sage_dynamic_tiles.py's float64 bound computed from the 16-bit values — one
  shape per launch branch (lane groups of 8 / 16 / 32 / 64, compile-time consumers, 32-row tiles, half tiles with one and four
  multiplying waves), ReLU on and off.  209 rows: three 64-row tiles and a partial one; degrees 0, <= 10, 11..26 and > 26 (both
  neighbour windows and the long-row loop).  Planted values: fp16 subnormals, -0.0, +-65504; bf16 2^-120 and 2^100.
* the training entry (``agg_out``): output and kept aggregate equal the float32 route's.
* ``nn.SAGEConv`` over a two-hop ``LayerGraph`` with ``LazyRows(table16, n_id)``: forward equal to the float32 table's, weight
  and bias gradients within tests/test_gpu_sage_train.py's float64 bounds, a gradient into the table refused.
* rows that are 8-B but not 16-B aligned; ``precision="f32"`` and byte-offset ids refused.
* GCNConv / GATConv over the same ``LazyRows``: float32 rows from the converting gather, equal to ``table16.float()[n_id]``."""
import functools

import numpy as np
import pytest

from graphgen import powerlaw_csr
from layer_graphs import empty_hop_graph

pytestmark = pytest.mark.gpu

# F -> N: the launch branch
SHAPES = [(20, 64),      # lane groups of 8, one multiplying wave
          (64, 128),     # lane groups of 16
          (100, 256),    # lane groups of 32, compile-time consumer
          (128, 256),    # lane groups of 32, compile-time consumer
          (132, 64),     # lane groups of 64, 32-row tiles
          (256, 47),     # half tiles, padded head: the multiplying wave reads 16-bit self rows
          (160, 256)]    # half tiles, four multiplying waves
N_ROWS = 209
DTYPES = ["float16", "bfloat16"]


def _dtype(name):
    import torch
    return getattr(torch, name)


def _planted(name):
    """Rows of special values (one value per row, repeated over the row with alternating neighbours kept finite)."""
    if name == "float16":
        return [6e-8, -6e-8, 3e-5, -3e-5, -0.0, 65504.0, -65504.0]      # subnormals (2^-24, ~2^-15), -0, the largest normal
    return [2.0 ** -120, -(2.0 ** -120), 2.0 ** 100, -(2.0 ** 100), -0.0]


@functools.lru_cache(maxsize=None)
def _graph():
    rp, col = powerlaw_csr(N_ROWS, 8, seed=5, col_dtype=np.int32, max_deg=60)
    deg = np.diff(rp)
    deg[[5, 70, N_ROWS - 1]] = 0              # rows without neighbours, the last row of the partial tile among them
    rp = np.concatenate([[0], np.cumsum(deg)])
    col = col[:rp[-1]].copy()
    assert (deg == 0).any() and ((deg > 0) & (deg <= 10)).any() and ((deg > 10) & (deg <= 26)).any() and (deg > 26).any()
    return rp.astype(np.int32), col


@functools.lru_cache(maxsize=None)
def _case(F, N, name):
    """Inputs on the device, the float64 result (before the activation) and its error scale; never modified."""
    import torch
    dt = _dtype(name)
    rp, col = _graph()
    rng = np.random.default_rng(1000 * F + N + len(name))
    n_src, V = N_ROWS, 3 * N_ROWS
    cu = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    table = cu(rng.standard_normal((V, F)).astype(np.float32)).to(dt)
    ids = rng.permutation(V)[:n_src].astype(np.int64)
    self_rows = rng.integers(0, n_src, N_ROWS).astype(np.int64)
    # planted rows: node-list positions 0 .. P-1, each read as the first neighbour of a destination row of its own (two of them
    # in one sum would cancel) and as a self row
    vals = _planted(name)
    col = col.copy()
    for p, v in enumerate(vals):
        row = torch.full((F,), v, dtype=torch.float64)
        row[1::3] = 0.5                                  # (the row is not constant: a lane reading its neighbour's features shows)
        table[ids[p]] = row.to(dt).cuda()
        dst = 10 + 3 * p
        assert rp[dst + 1] > rp[dst]
        col[rp[dst]], self_rows[7 * p + 1] = p, p
    assert not bool(torch.isinf(table.float()).any() | torch.isnan(table.float()).any())
    if name == "float16":
        assert bool(((table.float().abs() < 2.0 ** -14) & (table.float() != 0)).any()), "no fp16 subnormal planted"
    w_t = cu((rng.standard_normal((2 * F, N)) * 0.2).astype(np.float32))
    bias = cu(rng.standard_normal(N).astype(np.float32))
    rp, col, ids, self_rows = cu(rp), cu(col), cu(ids), cu(self_rows)
    x64 = table[ids].double()                                       # exact: every 16-bit value is a float64
    deg = (rp[1:] - rp[:-1]).long()
    owner = torch.repeat_interleave(torch.arange(N_ROWS, device="cuda"), deg)
    agg = torch.zeros((N_ROWS, F), dtype=torch.float64, device="cuda").index_add_(0, owner, x64[col.long()])
    agg /= deg.clamp(min=1).unsqueeze(1)
    cat = torch.cat([agg, x64[self_rows]], 1)
    ref = cat @ w_t.double() + bias.double()
    scale = cat.abs() @ w_t.double().abs() + bias.double().abs()
    return dict(rp=rp, col=col, table=table, table32=table.float(), ids=ids, ids32=ids.int(), self_rows=self_rows, w_t=w_t,
                bias=bias, ref=ref, scale=scale, agg=agg)


def _run(c, table, ids, relu, **kw):
    from wholegraph_amd import nn
    return nn.sage_layer_fused_forward(c["rp"], c["col"], table, c["self_rows"], c["w_t"], c["bias"], relu=relu, mean=True,
                                       src_ids=ids, precision="bf16x3", **kw)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("ids", ["int32", "int64"])
@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("F,N", SHAPES)
def test_bit_for_bit_the_float32_route(hiplib, F, N, name, ids, relu):
    import torch
    from test_gpu_sage_dynamic_tiles import _check_fp64
    c = _case(F, N, name)
    idx = c["ids32"] if ids == "int32" else c["ids"]
    got = _run(c, c["table"], idx, relu)
    want = _run(c, c["table32"], idx, relu)
    assert got.dtype == torch.float32 and got.shape == (N_ROWS, N)
    assert torch.equal(got, want), "16-bit route differs from the float32 route: max |diff| %.3e" % float((got - want).abs().max())
    _check_fp64(got, c, N_ROWS, relu)


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("F,N", [(100, 256), (160, 256), (132, 64)])
def test_training_entry_output_and_aggregate(hiplib, F, N, name):
    import torch
    c = _case(F, N, name)
    agg16 = torch.full((N_ROWS, F), float("nan"), device="cuda")
    agg32 = torch.full((N_ROWS, F), float("nan"), device="cuda")
    out16 = _run(c, c["table"], c["ids"], True, agg_out=agg16)
    out32 = _run(c, c["table32"], c["ids"], True, agg_out=agg32)
    assert torch.equal(out16, out32) and torch.equal(agg16, agg32)
    assert torch.equal(out16, _run(c, c["table"], c["ids"], True)), "the training launch changes the output"
    ref = c["agg"]
    assert torch.all((agg16.double() - ref).abs() <= 1e-5 * ref.abs() + 1e-6)


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("F,N", [(100, 256), (160, 47)])
def test_sage_conv_lazy_rows_forward_and_gradients(hiplib, F, N, name):
    import torch
    from test_gpu_sage_train import _close, _ref_layer
    from wholegraph_amd import nn
    n_src, V = 300, 900
    lg, _, _ = empty_hop_graph(n_src, seed=F + N)
    g = torch.Generator(device="cuda").manual_seed(3 * F + N)
    table16 = torch.randn((V, F), generator=g, device="cuda").to(_dtype(name))
    n_id = torch.randperm(V, generator=g, device="cuda")[:n_src]
    torch.manual_seed(F * 7 + N)
    conv = nn.SAGEConv((F, F), N).cuda()
    x16, x32 = nn.LazyRows(table16, n_id), nn.LazyRows(table16.float(), n_id)
    with torch.no_grad():
        want = conv(x32, lg, act="relu").clone()
        assert torch.equal(conv(x16, lg, act="relu"), want)
    out = conv(x16, lg, act="relu")
    assert out.requires_grad and torch.equal(out, want)
    assert x16._rows is None, "the one-kernel route gathered the rows"
    gout = torch.randn(out.shape, generator=g, device="cuda")
    out.backward(gout)
    got = [p.grad.clone() for p in (conv.lin_l.weight, conv.lin_r.weight, conv.lin_l.bias)]
    # float64 autograd of the dense formula over the 16-bit values (tests/test_gpu_sage_train.py's bounds)
    hops = [(h.row_ptr, h.col, h.self_rows) for h in lg.hops]
    x64 = table16[n_id].double()
    wl, wr, b = (p.detach().double().requires_grad_(True) for p in (conv.lin_l.weight, conv.lin_r.weight, conv.lin_l.bias))
    pre = _ref_layer(x64, hops, wl, wr, b, False, True)
    fscale = _ref_layer(x64.abs(), hops, wl.detach().abs(), wr.detach().abs(), b.detach().abs(), False, True)
    mask = out.detach() > 0
    flip = mask != (pre.detach() > 0)
    assert bool((pre.detach().abs()[flip] <= 1e-5 * fscale[flip] + 1e-7).all()), "ReLU mask differs away from the kink"
    ref = pre * mask
    ref.backward(gout.double())
    _close(out.detach(), ref.detach(), fscale, "forward")
    dz = gout.double() * mask
    wla, wra, ba = (t.detach().abs().requires_grad_(True) for t in (wl, wr, b))
    _ref_layer(x64.abs(), hops, wla, wra, ba, False, True).backward(dz.abs())
    _close(got[0], wl.grad, wla.grad, "grad lin_l.weight")
    _close(got[1], wr.grad, wra.grad, "grad lin_r.weight")
    _close(got[2], b.grad, ba.grad, "grad bias")
    # a gradient into the table stays refused, with the message of the float32 table
    t_grad = table16.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="gradient w.r.t. a feature table read through ids"):
        conv(nn.LazyRows(t_grad, n_id), lg, act="relu")


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("F,N", [(100, 256), (160, 64)])
def test_rows_aligned_to_8_bytes_only(hiplib, F, N, name):
    """A [V, F] view with a row stride of ``ldx % 8 == 4`` elements that starts 8 bytes into its buffer: the base and every other
    row are 8-B but not 16-B aligned."""
    import torch
    c = _case(F, N, name)
    V, ld = c["table"].shape[0], (F + 4 if (F + 4) % 8 == 4 else F + 8)
    assert ld % 8 == 4
    buf = torch.zeros(V * ld + 8, dtype=c["table"].dtype, device="cuda")
    view = buf[4:4 + V * ld].view(V, ld)[:, :F]
    view.copy_(c["table"])
    assert view.data_ptr() % 16 == 8 and view.stride(0) == ld
    for relu in (False, True):
        assert torch.equal(_run(c, view, c["ids"], relu), _run(c, c["table32"], c["ids"], relu))


def test_refusals(hiplib):
    import torch
    from wholegraph_amd import _lib as L
    from wholegraph_amd import nn
    from wholegraph_amd.env import get_stream
    c = _case(100, 256, "float16")
    with pytest.raises((ValueError, AssertionError)):
        nn.sage_layer_fused_forward(c["rp"], c["col"], c["table"], c["self_rows"], c["w_t"], c["bias"], src_ids=c["ids"], precision="f32")

    class Mapped16(nn.MappedTable):         # what a peer-mapped 16-bit table would look like: byte-offset ids
        dtype = torch.float16
    offs = c["ids"] * (100 * 2)
    with pytest.raises((ValueError, AssertionError, RuntimeError)):
        nn.sage_layer_fused_forward(c["rp"], c["col"], Mapped16(c["table"].data_ptr(), 100, c["table"].device), c["self_rows"],
                                    c["w_t"], c["bias"], src_ids=offs, precision="bf16x3")
    # the entry point itself says no before it launches anything
    planes = nn.sage_weight_planes(c["w_t"])
    out = torch.empty((N_ROWS, 256), device="cuda")
    rc = L.lib().wgamd_sage_layer_fused_bf16x3_x(
        c["rp"].data_ptr(), c["col"].data_ptr(), N_ROWS, c["table"].data_ptr(), L.DT_HALF, 100, c["table"].shape[0], 100,
        offs.data_ptr(), L.IDS_BYTE_OFFSETS, c["self_rows"].data_ptr(), 1, planes.data_ptr(), 256, c["bias"].data_ptr(), 0,
        out.data_ptr(), 256, get_stream())
    assert rc != 0
    assert L.lib().wgamd_sage_layer_x16_supported(100, 256, L.DT_HALF) == 1 and L.lib().wgamd_sage_layer_x16_supported(100, 256, L.DT_BF16) == 1
    assert L.lib().wgamd_sage_layer_x16_supported(100, 256, L.DT_DOUBLE) == 0 and L.lib().wgamd_sage_layer_x16_supported(101, 256, L.DT_HALF) == 0


@pytest.mark.parametrize("name", DTYPES)
def test_other_layers_get_float32_rows(hiplib, name):
    import torch
    from wholegraph_amd import nn
    F, n_src, V = 64, 300, 900
    lg, _, _ = empty_hop_graph(n_src, seed=21)
    lg.degree_source = lambda: (lg.hops, [-1, -1], n_src)      # (GCNConv's degrees, as tests/test_gpu_layer_empty_hop.py sets them)
    g = torch.Generator(device="cuda").manual_seed(22)
    table16 = torch.randn((V, F), generator=g, device="cuda").to(_dtype(name))
    n_id = torch.randperm(V, generator=g, device="cuda")[:n_src]
    rows32 = table16.float()[n_id]
    lazy = nn.LazyRows(table16, n_id)
    assert lazy.dtype == table16.dtype
    torch.manual_seed(23)
    gcn, gat = nn.GCNConv(F, 64).cuda(), nn.GATConv(F, 16, heads=4).cuda()
    with torch.no_grad():
        assert torch.equal(gcn(nn.LazyRows(table16, n_id), lg), gcn(rows32, lg))
        assert torch.equal(gat(nn.LazyRows(table16, n_id), lg), gat(rows32, lg))
    rows = lazy.materialize()
    assert rows.dtype == torch.float32 and torch.equal(rows, rows32) and lazy.materialize() is rows
    assert lazy.dtype == table16.dtype
