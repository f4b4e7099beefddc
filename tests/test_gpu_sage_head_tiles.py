"""The 64-column head of the one-kernel SAGE layer in half-tile mode (F = 256 -> 47 / 64): four multiplying waves per
workgroup, wave w owning the 32 x 32 accumulator (row tile w >> 1, column tile w & 1) of the 64 x 64 output tile.

Every output element goes through the chain of MFMAs it goes through in the N = 256 half-tile launch — same A, same k order,
same six products — so column c of a launch with the first 47 or 64 columns of a 256-column weight must equal column c of the
launch with the whole weight BIT FOR BIT.  That launch (four waves of 64 columns each) is the reference the equality is held
against; the float64 bounds of tests/test_gpu_aggregate.py hold the values themselves, with weights whose second column tile
is 2^8 larger than the first, so that a swapped or shifted column tile breaks the bound and not only the equality.

Row counts (C = compute units): 41 (one partial tile), 64 C + 1, 64 (2 C + 3) + 17, and two tails — 64 k + 33 (the last tile's
second row tile holds ONE live row) and 64 k + 32 (it holds none).  Every row count is a prefix of ONE graph (rows of degree
0, rows past both neighbour windows), one float64 reference serves them all."""
import functools

import numpy as np
import pytest

from graphgen import powerlaw_csr

pytestmark = pytest.mark.gpu

F, NW = 256, 256


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _row_counts():
    C = _cus()
    return {"partial": 41, "64C+1": 64 * C + 1, "rounds": 64 * (2 * C + 3) + 17}


def _tail_counts():
    k = _cus() + 2
    return {"one_live_row": 64 * k + 33, "empty_row_tile": 64 * k + 32}


def _dtype(name):
    import torch
    return {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[name]


@functools.lru_cache(maxsize=None)
def _graph():
    import torch
    n_max = max(_row_counts().values())
    rp, col = powerlaw_csr(n_max, 8, seed=F + 47, col_dtype=np.int32, max_deg=60)
    rng = np.random.default_rng(5 * F + 47)
    cu = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    # (the generator gives every row an edge at these parameters: every 29th row is emptied, the last row among them)
    deg = np.diff(rp)
    keep = np.repeat((np.arange(n_max) % 29 != (n_max - 1) % 29), deg)
    deg[(n_max - 1) % 29::29] = 0
    rp, col = np.concatenate([[0], np.cumsum(deg)]), col[keep]
    assert rp[-1] == col.shape[0] and (deg[:41] == 0).any() and (deg == 0).any() and (deg > 26).any(), "degree 0 and rows past both neighbour windows"
    return dict(n=n_max, rp=cu(rp.astype(np.int32)), col=cu(col), self_rows=cu(rng.integers(0, n_max, n_max).astype(np.int64)),
                w_t=cu((rng.standard_normal((2 * F, NW)) * 0.2).astype(np.float32)), bias=cu(rng.standard_normal(NW).astype(np.float32)),
                perm=cu(rng.permutation(3 * n_max)[:n_max].astype(np.int32)),
                values=cu(rng.standard_normal((3 * n_max, F)).astype(np.float32)))


@functools.lru_cache(maxsize=None)
def _table(dtype, with_ids):
    """(x, src_ids): the feature table as stored; rows [0, n) of the layer's input are x[src_ids] or x itself."""
    g = _graph()
    if with_ids:
        return g["values"].to(_dtype(dtype)), g["perm"]
    return g["values"][g["perm"].long()].to(_dtype(dtype)).contiguous(), None


def _run(n, w_t, bias, relu, dtype="f32", with_ids=False, **kw):
    from wholegraph_amd import nn
    g = _graph()
    x, ids = _table(dtype, with_ids)
    return nn.sage_layer_fused_forward(g["rp"][:n + 1], g["col"], x, g["self_rows"][:n].contiguous(), w_t, bias, relu=relu,
                                       mean=True, src_ids=ids, precision="bf16x3", **kw)


@functools.lru_cache(maxsize=None)
def _wide(n, relu, dtype, with_ids):
    """The N = 256 half-tile launch (four multiplying waves of 64 columns): the path the head is held against; never modified."""
    g = _graph()
    return _run(n, g["w_t"], g["bias"], relu, dtype, with_ids)


@pytest.mark.parametrize("cols", [47, 64])
@pytest.mark.parametrize("with_ids", [False, True], ids=["rows", "int32_ids"])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("rows", ["partial", "64C+1", "rounds"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_head_columns_equal_the_wide_launch_bit_for_bit(hiplib, dtype, rows, relu, with_ids, cols):
    import torch
    g, n = _graph(), _row_counts()[rows]
    got = _run(n, g["w_t"][:, :cols], g["bias"][:cols], relu, dtype, with_ids)
    assert got.shape == (n, cols)
    assert torch.equal(got, _wide(n, relu, dtype, with_ids)[:, :cols])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_training_entry_keeps_the_bits_and_the_aggregate(hiplib, dtype):
    import torch
    from wholegraph_amd import nn
    g, n = _graph(), _row_counts()["rounds"]
    assert nn.sage_layer_train_supported(F, 47)
    agg = torch.full((n, F), float("nan"), device="cuda")
    out = _run(n, g["w_t"][:, :47], g["bias"][:47], True, dtype, agg_out=agg)
    assert torch.equal(out, _run(n, g["w_t"][:, :47], g["bias"][:47], True, dtype))
    assert torch.equal(out, _wide(n, True, dtype, False)[:, :47])
    x64 = _table(dtype, False)[0].double()
    deg = (g["rp"][1:n + 1] - g["rp"][:n]).long()
    owner = torch.repeat_interleave(torch.arange(n, device="cuda"), deg)
    ref = torch.zeros((n, F), dtype=torch.float64, device="cuda").index_add_(0, owner, x64[g["col"][:int(deg.sum())].long()])
    ref /= deg.clamp(min=1).unsqueeze(1)
    assert torch.all((agg.double() - ref).abs() <= 1e-5 * ref.abs() + 1e-6)


@pytest.mark.parametrize("relu", [True, False])
def test_fp64_bounds_with_column_tiles_of_different_scale(hiplib, relu):
    """tests/test_gpu_aggregate.py's bounds on the 47-column result at the largest row count: |err| <= 1e-5 * sum |a||b| + 1e-6
    everywhere, and 1e-5 relative wherever the result is not a cancellation (|ref| >= 0.1 * scale).  Columns 32..46 — the second
    column tile — carry weights and a bias 2^8 times those of columns 0..31."""
    import torch
    g, n = _graph(), _row_counts()["rounds"]
    gain = torch.ones(47, device="cuda")
    gain[32:] = 256.0
    w_t, bias = (g["w_t"][:, :47] * gain).contiguous(), (g["bias"][:47] * gain).contiguous()
    got = _run(n, w_t, bias, relu)
    x64 = _table("f32", False)[0].double()
    deg = (g["rp"][1:n + 1] - g["rp"][:n]).long()
    owner = torch.repeat_interleave(torch.arange(n, device="cuda"), deg)
    agg = torch.zeros((n, F), dtype=torch.float64, device="cuda").index_add_(0, owner, x64[g["col"][:int(deg.sum())].long()])
    agg /= deg.clamp(min=1).unsqueeze(1)
    cat = torch.cat([agg, x64[g["self_rows"][:n]]], 1)
    ref = cat @ w_t.double() + bias.double()
    scale = cat.abs() @ w_t.double().abs() + bias.double().abs()
    if relu:
        ref = ref.clamp(min=0)
    err = (got.double() - ref).abs()
    big = ref.abs() >= 0.1 * scale
    print("max err %.3e, max err / bound %.3f, max rel %.3e" % (float(err.max()), float((err / (1e-5 * scale + 1e-6)).max()),
                                                                  float((err[big] / ref.abs()[big]).max())))
    assert torch.all(err <= 1e-5 * scale + 1e-6), float(err.max())
    assert bool(big[:, :32].any()) and bool(big[:, 32:].any()) and float((err[big] / ref.abs()[big]).max()) <= 1e-5


@pytest.mark.parametrize("cols", [47, 64])
@pytest.mark.parametrize("rows", ["one_live_row", "empty_row_tile"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_tail_rows_and_untouched_rows_past_the_end(hiplib, dtype, rows, cols):
    import torch
    g, n = _graph(), _tail_counts()[rows]
    sentinel = -12345.0
    buf = torch.full((n + 96, 64), sentinel, device="cuda")     # the head runs at 64 columns: `out` is a view of the padded buffer
    got = _run(n, g["w_t"][:, :cols], g["bias"][:cols], False, dtype, out=buf[:n, :cols])
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[:n, :cols], _wide(n, False, dtype, False)[:, :cols])
    assert bool((buf[n:] == sentinel).all()), "rows past n_rows were written"
