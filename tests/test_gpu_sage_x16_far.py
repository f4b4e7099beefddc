"""The one-kernel SAGE layer over a float16 / bfloat16 table larger than 2^31 and 2^32 bytes: a 16-bit [rows, 100] view of the far
buffer of tests/far_offsets.py (16 GiB of NaN, a few hundred live rows), read through int64 ids that name rows on both sides of
byte 2^31, byte 2^32 (= element 2^31) and byte 2^33 (= element 2^32).  A table of that size takes the kernel's 64-bit addressing
path, whose byte offset of a row is ``id * (2 * ldx)``: a truncated product or a lost high word reads the NaN fill or another
live row's different numbers.  The result must equal, bit for bit, the float32 route over the gathered live rows."""
import numpy as np
import pytest

import far_offsets as fo

pytestmark = pytest.mark.gpu

F, N_DST = 100, 150


@pytest.fixture(scope="module", autouse=True)
def _memory():
    ok, why = fo.enough_memory()
    if not ok:
        pytest.skip(why)


@pytest.fixture(scope="module")
def far(_memory):
    import torch
    buf = fo.far_buffer()
    torch.cuda.synchronize()
    yield buf
    del buf
    torch.cuda.empty_cache()


def _live_rows():
    """``band_rows(100, 2, per_band=2)`` — two rows on either side of every threshold, row 0 and the last row — plus a couple of
    hundred rows spread over the view.  ``band_rows`` requires that a spread row's position, wrapped modulo 2^31 or 2^32 bytes or
    elements, lands on the NaN fill and on no other live row: the few candidates that would are left out."""
    band = set(fo.band_rows(F, 2, per_band=2).tolist())
    extra = [r for r in fo.spread_rows(F, 2, low=120, high=120) if r not in band]
    while True:
        rows = np.array(sorted(band | set(extra)), dtype=np.int64)
        hit = {x for r, _, s in fo.wrap_collisions(rows, F, 2) for x in (r, s)} - band
        if not hit:
            return fo.band_rows(F, 2, per_band=2, more=extra)
        extra = [r for r in extra if r not in hit]


def _hop(n_src, seed):
    """150 destinations over ``n_src`` input rows: degrees 0 .. 40 (both neighbour windows and the long-row loop), every input
    row read at least once."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    deg = torch.randint(0, 41, (N_DST,), generator=g, device="cuda")
    deg[:4] = torch.tensor([0, 1, 26, 40], device="cuda")
    rp = torch.zeros(N_DST + 1, dtype=torch.int32, device="cuda")
    rp[1:] = torch.cumsum(deg, 0)
    E = int(rp[-1])
    assert E >= n_src
    col = torch.randint(0, n_src, (E,), generator=g, device="cuda", dtype=torch.int32)
    col[torch.randperm(E, generator=g, device="cuda")[:n_src]] = torch.arange(n_src, device="cuda", dtype=torch.int32)
    self_rows = torch.randint(0, n_src, (N_DST,), generator=g, device="cuda")
    return rp, col, self_rows


@pytest.mark.parametrize("N", [256, 64])
@pytest.mark.parametrize("name", ["float16", "bfloat16"])
def test_16_bit_rows_beyond_2_and_4_gib(hiplib, far, name, N):
    import torch
    from wholegraph_amd import nn
    dtype = getattr(torch, name)
    v = fo.view(far, F, dtype)
    assert v.data_ptr() == far.data_ptr() and v.shape[0] * F * 2 > (1 << 33)
    rows = _live_rows()
    L = F * 2
    for T in (1 << 31, 1 << 32, 1 << 33):       # live rows on both sides of every threshold
        assert (rows * L < T).any() and ((rows * L >= T) & (rows * L < T + 2 * L)).any() and (((rows + 1) * L <= T) & (rows * L >= T - 2 * L)).any()
    n_src = len(rows)
    assert 200 <= n_src <= 400
    g = torch.Generator(device="cuda").manual_seed(N + len(name))
    vals = torch.randn((n_src, F), generator=g, device="cuda").to(dtype)       # (pairwise different rows: checked by place)
    w_t = torch.randn((2 * F, N), generator=g, device="cuda") * 0.2
    bias = torch.randn(N, generator=g, device="cuda")
    rp, col, self_rows = _hop(n_src, N)
    ids = torch.from_numpy(rows).cuda()
    assert ids.dtype == torch.int64
    run = lambda table, src_ids, **kw: nn.sage_layer_fused_forward(rp, col, table, self_rows, w_t, bias, relu=True, src_ids=src_ids,  # noqa: E731
                                                                  precision="bf16x3", **kw)
    want = run(vals.float(), None)
    assert bool(torch.isfinite(want).all())
    fo.place(v, rows, vals)
    try:
        got = run(v, ids)
        agg16, agg32 = torch.empty((N_DST, F), device="cuda"), torch.empty((N_DST, F), device="cuda")
        got_train = run(v, ids, agg_out=agg16)
        run(vals.float(), None, agg_out=agg32)
        torch.cuda.synchronize()
    finally:
        fo.clear(v, rows)
    assert fo.is_fill(v, rows)
    assert torch.equal(got, want), "rows read from the wrong place: %d elements differ" % int((got != want).sum())
    assert torch.equal(got_train, want) and torch.equal(agg16, agg32)
