"""Tables, CSR arrays and outputs whose rows lie beyond 2^31 and 2^32 bytes, and beyond element 2^31 and 2^32, from their base
pointer — the offsets papers100m (56.9 GB of features, 13.7 GB of CSR) and rmat26 run at, which no other test reaches.

Scheme of every case (tests/far_offsets.py): the table is a view of ONE 16 GiB + 256 KiB allocation filled with NaN, a few
dozen of its rows are live — rows that straddle byte offset 2^31, byte offset 2^32, element 2^31 and element 2^32, row 0, the
last row, a few in between — and a small hop (333 destinations: several 16-, 32- and 64-row tiles and a ragged last one; degrees
0 .. 40 and a hub of 90, past the kernels' register and prefetch windows) reads them through a node list.  The result must be
(a) bit for bit what the same entry point gives on the compact copy of those rows, read directly and through ``arange`` — a
kernel that truncates an offset reads NaN or another row's numbers instead — and (b) within the bound the kernel's own test
file uses of the float64 formula on the compact copy.  The embedding tables (4 GiB + 32 KiB each) are allocations of their
own, made and freed before the far buffer exists; the weighted hop adds an 8 GiB weights array for its own duration."""
import contextlib

import numpy as np
import pytest

import far_offsets as fo

pytestmark = pytest.mark.gpu

N_DST = 333


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


@contextlib.contextmanager
def live(v, rows, values):
    """``values`` in rows ``rows`` of the far view ``v`` for the duration of a case."""
    fo.place(v, rows, values)
    try:
        yield
    finally:
        fo.clear(v, rows)


def _hop(n_src, seed, n_dst=N_DST, distinct_self_rows=False):
    """A hop over ``n_src`` input rows: every input row is read at least once, the last ones by the hub and as self rows.
    ``distinct_self_rows``: no two destinations share an input row (what a sampled hop guarantees and the input gradient over
    ``HopGraph.transposed`` relies on); otherwise rows repeat, as the forward kernels allow."""
    import torch
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 41, n_dst)
    deg[:5] = [0, 1, 40, 90, 10]
    deg[-1] = 11
    rp = np.zeros(n_dst + 1, np.int32)
    rp[1:] = np.cumsum(deg)
    E = int(rp[-1])
    col = rng.integers(0, n_src, E).astype(np.int32)
    assert E >= 2 * n_src
    col[rng.permutation(E)[:n_src]] = np.arange(n_src, dtype=np.int32)
    self_rows = rng.integers(0, n_src, n_dst).astype(np.int64)
    self_rows[:n_src] = rng.permutation(n_src)[:n_dst]
    if distinct_self_rows:
        assert n_src >= n_dst
        self_rows = rng.permutation(n_src)[:n_dst].astype(np.int64)
    return torch.from_numpy(rp).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(self_rows).cuda()


def _values(n, F, seed, dtype=None):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn((n, F), generator=g, device="cuda").to(dtype or torch.float32)


def _ids(rows, dtype):
    import torch
    return torch.from_numpy(np.asarray(rows)).to(dtype).cuda()


def _close(got, ref, scale, what, floor=1e-6):
    """|err| <= 1e-5 x the magnitude sum of the terms (tests/test_gpu_aggregate.py, test_gpu_gcn.py, test_gpu_sage_train.py)."""
    import torch
    err = (got.double() - ref).abs()
    print(what, "max err %.3e, max err / bound %.3f" % (float(err.max()), float((err / (1e-5 * scale + floor)).max())))
    assert bool(torch.isfinite(got).all()), what
    assert bool((err <= 1e-5 * scale + floor).all()), (what, float(err.max()))


def _same(a, b, what):
    import torch
    assert a.shape == b.shape and torch.equal(a, b), "%s: %d of %d elements differ, %d are NaN" % (
        what, int((a != b).sum()), a.numel(), int(torch.isnan(a.float()).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# embedding apply: tables of their own, before the far buffer exists
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
def test_embedding_apply_on_a_table_past_4_gib(oracle_mod, hiplib, opt):
    """wg_embedding.hip on a single-rank fp32 table of 8,388,608 + 64 rows x 128 (4 GiB + 32 KiB; adagrad's state table is as
    large): gradient rows around byte 2^31 and 2^32 with duplicates and negative ids, against the oracle's optimiser step on the
    compact rows at test_gpu_embedding.py's bound; the rows beside the updated ones keep their bits."""
    import torch
    import wholegraph_amd as wg
    from oracle import embedding_optimizer as eo
    from test_gpu_embedding import _close as close_embedding
    n, dim = 8_388_608 + 64, 128
    comm = wg.create_group_communicator()
    emb = wg.create_embedding(comm, "distributed", "cuda", torch.float32, [n, dim])
    optimizer = wg.create_wholememory_optimizer(emb, opt, {})
    try:
        local = emb.get_embedding_tensor().get_local_tensor()[0]
        assert tuple(local.shape) == (n, dim) and local.stride(0) == dim and n * dim * 4 == (1 << 32) + (1 << 15)
        local.fill_(float("nan"))
        rows = fo.band_rows(dim, 4, 3, n_bytes=n * dim * 4)
        assert any(r * dim * 4 == 1 << 31 for r in rows) and any(r * dim * 4 == 1 << 32 for r in rows) and rows[-1] == n - 1
        near = fo.neighbours(rows, n)
        rng = np.random.default_rng(len(opt))
        start = rng.uniform(-10, 10, (len(rows), dim)).astype(np.float32)
        fo.place(local, rows, start)
        states = {name: emb.get_optimizer_state(name).get_local_tensor()[0] for name in eo.STATE_NAMES[opt]}
        near_t = torch.from_numpy(near).cuda()
        rows_t = torch.from_numpy(rows).cuda()
        states_before = {name: s[near_t].clone() for name, s in states.items()}
        cpu = eo.SparseOptimizer(opt, len(rows), dim)
        ref = start.copy()
        for step in range(3):
            pick = rng.integers(0, len(rows), 400)                 # 400 gradient rows over a few dozen ids: duplicates
            pick[:len(rows)] = np.arange(len(rows))
            idx, compact = rows[pick].copy(), pick.copy()
            idx[::7], compact[::7] = -1, -1
            grads = rng.uniform(-5, 5, (400, dim)).astype(np.float32)
            emb.add_gradients(torch.from_numpy(idx).to(torch.int32 if step == 1 else torch.int64).cuda(), torch.from_numpy(grads).cuda())
            emb.need_apply = True
            optimizer.step(0.1)
            cpu.step(ref, compact, grads, 0.1)
        close_embedding(local[rows_t].cpu().numpy(), ref, start, 1e-5)
        assert fo.is_fill(local, near), "a row beside an updated one changed"
        for name, want in cpu.states.items():
            got = states[name][rows_t].cpu().numpy()
            assert got.shape == want.shape
            close_embedding(got, want, want, 1e-5)
            assert torch.equal(states[name][near_t].view(torch.int32), states_before[name].view(torch.int32)), "a state row beside an updated one changed"
        del local, states, states_before
    finally:
        wg.destroy_embedding(emb)
        wg.destroy_wholememory_optimizer(optimizer)
        comm.destroy()
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# gather and scatter (wg_gather.hip, wg_gather_terms.hip)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,table_dt,out_dt", [(100, "float32", "float32"), (128, "float32", "float32"),
                                               (128, "float16", "float32"), (128, "float16", "float16")])
def test_gather_and_scatter_band_rows(hiplib, far, F, table_dt, out_dt):
    """local_gather / local_scatter (wholememory_gather / _scatter): copying and converting paths, int32 and int64 ids."""
    import torch
    from wholegraph_amd.tensor import local_gather, local_scatter
    tdt, odt = getattr(torch, table_dt), getattr(torch, out_dt)
    v = fo.view(far, F, tdt)
    rows = fo.live_rows(F, v.element_size())
    vals = _values(len(rows), F, F, tdt)
    order = torch.from_numpy(np.random.default_rng(F).integers(0, len(rows), 700)).cuda()     # repeats, any order
    order[:len(rows)] = torch.arange(len(rows), device="cuda")
    assert int(rows[-1]) < 2**31
    with live(v, rows, vals):
        for idt in (torch.int32, torch.int64):
            ids = _ids(rows, idt)[order]
            got = local_gather(v, ids, torch.full((700, F), 7.0, dtype=odt, device="cuda"))
            want = local_gather(vals, order.to(idt), torch.full((700, F), 7.0, dtype=odt, device="cuda"))
            _same(got, want, "gather %s" % idt)
            _same(got, vals[order].to(odt), "gather vs indexing")           # fp16 -> fp32 is exact
    near = fo.neighbours(rows, v.shape[0])
    assert fo.is_fill(v, rows) and fo.is_fill(v, near)
    # scatter: distinct rows (one writer per row), read back with plain indexing; the rows next to them stay NaN
    src = _values(len(rows), F, F + 1, odt)
    try:
        for idt in (torch.int32, torch.int64):
            local_scatter(src, _ids(rows, idt), v)
            torch.cuda.synchronize()
            _same(v[torch.from_numpy(rows).cuda()], src.to(tdt), "scatter %s" % idt)
            assert fo.is_fill(v, near), "scatter wrote a row next to its target"
            fo.clear(v, rows)
    finally:
        fo.clear(v, rows)


@pytest.mark.parametrize("F,T", [(128, 8), (64, 20)])
def test_gather_with_terms_band_rows(hiplib, far, F, T):
    """gather_with_terms / lazy_rows_terms (wgamd_gather_terms_f32): rows bit for bit, terms bit for bit the compact run's and
    within 1e-5 x scale of the float64 product (test_gpu_mag_pipeline.py)."""
    import torch
    from wholegraph_amd import nn
    v = fo.view(far, F, torch.float32)
    rows = fo.live_rows(F, 4)
    vals = _values(len(rows), F, F + T)
    w = _values(F, T, 3) * 0.3
    order = torch.from_numpy(np.random.default_rng(T).integers(0, len(rows), 500)).cuda()
    order[:len(rows)] = torch.arange(len(rows), device="cuda")
    x0, t0 = nn.gather_with_terms(vals, order, w)
    _same(x0, vals[order], "compact rows")
    _close(t0, vals[order].double() @ w.double(), vals[order].double().abs() @ w.double().abs(), "terms", floor=1e-7)
    with live(v, rows, vals):
        for idt in (torch.int32, torch.int64):
            ids = _ids(rows, idt)[order]
            x1, t1 = nn.gather_with_terms(v, ids, w)
            _same(x1, x0, "rows %s" % idt)
            _same(t1, t0, "terms %s" % idt)
            _same(nn.lazy_rows_terms(v, ids, w), t0, "lazy terms %s" % idt)
            if T % 4 == 0:
                _same(nn.lazy_rows_terms(v, ids, w, heads=4), nn.lazy_rows_terms(vals, order, w, heads=4), "slabs %s" % idt)


def test_gather_term_slabs_band_rows(hiplib, far):
    """gather_term_slabs (wgamd_gather_term_slabs_f32) over [K, n, 4] slabs that fill the far buffer: the ids whose entry in
    some slab straddles a threshold, the first and the last id."""
    import torch
    from wholegraph_amd import nn
    K = 4
    n_in = fo.N_ELEMS // (4 * K)
    slabs = far[:K * n_in * 4].view(K, n_in, 4)
    flat = far[:K * n_in * 4].view(K * n_in, 4)
    ids = {0, n_in - 1}
    for T in fo.thresholds(4):
        for k in range(K):
            r = T // 16 - k * n_in
            ids.update(i for i in range(r - 2, r + 2) if 0 <= i < n_in)
    ids = np.array(sorted(ids), dtype=np.int64)
    assert 10 <= len(ids) <= 60
    rows = (np.arange(K, dtype=np.int64)[:, None] * n_in + ids[None, :]).reshape(-1)
    vals = _values(len(rows), 4, 9)
    order = torch.from_numpy(np.random.default_rng(1).integers(0, len(ids), 300)).cuda()
    compact = vals.view(K, len(ids), 4).contiguous()
    want = nn.gather_term_slabs(compact, order)
    _same(want, compact[:, order], "compact slabs")
    with live(flat, rows, vals):
        for idt in (torch.int32, torch.int64):
            _same(nn.gather_term_slabs(slabs, _ids(ids, idt)[order]), want, "slabs %s" % idt)


# ---------------------------------------------------------------------------------------------------------------------
# aggregates
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [100, 128])
def test_aggregates_band_rows(oracle_mod, hiplib, far, F):
    """spmm_csr_forward(src_ids=...) and sage_aggregate_fetch_forward against the oracle's sequential fp32 SpMM (bit for bit, as
    tests/test_gpu_aggregate.py has it) and its float64 one."""
    import torch
    from wholegraph_amd import nn
    v = fo.view(far, F, torch.float32)
    rows = fo.live_rows(F, 4)
    n_src = len(rows)
    vals = _values(n_src, F, F + 7)
    rp, col, self_rows = _hop(n_src, F)
    ar = torch.arange(n_src, device="cuda")
    for mean in (True, False):
        ref32 = oracle_mod.spmm_csr(rp.cpu().numpy(), col.cpu().numpy(), vals.cpu().numpy(), mean=mean, acc_double=False)
        ref64 = oracle_mod.spmm_csr(rp.cpu().numpy(), col.cpu().numpy(), vals.cpu().numpy(), mean=mean, acc_double=True)
        base = nn.spmm_csr_forward(rp, col, vals, mean)
        assert np.array_equal(base.cpu().numpy(), ref32)
        np.testing.assert_allclose(base.cpu().numpy(), ref64, rtol=1e-5, atol=1e-6 * 90)
        _same(nn.spmm_csr_forward(rp, col, vals, mean, src_ids=ar), base, "arange")
        cat = nn.sage_aggregate_fetch_forward(rp, col, vals, ar, self_rows, mean)
        assert np.array_equal(cat[:, :F].cpu().numpy(), ref32) and torch.equal(cat[:, F:], vals[self_rows])
        with live(v, rows, vals):
            for idt in (torch.int32, torch.int64):
                ids = _ids(rows, idt)
                _same(nn.spmm_csr_forward(rp, col, v, mean, src_ids=ids), base, "spmm %s" % idt)
                _same(nn.sage_aggregate_fetch_forward(rp, col, v, ids, self_rows, mean), cat, "sage aggregate %s" % idt)


# ---------------------------------------------------------------------------------------------------------------------
# the one-kernel SAGE layer (wg_sage_mfma*.h*, wg_sage_fused.hip)
# ---------------------------------------------------------------------------------------------------------------------
def _sage_ref(rp, col, self_rows, x, w_t, bias, relu):
    import torch
    deg = (rp[1:] - rp[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(rp.shape[0] - 1, device="cuda"), deg)
    x64 = x.double()
    agg = torch.zeros((rp.shape[0] - 1, x.shape[1]), dtype=torch.float64, device="cuda").index_add_(0, dst, x64[col.long()])
    agg = agg / deg.clamp(min=1).double().unsqueeze(1)
    cat = torch.cat([agg, x64[self_rows]], 1)
    ref = cat @ w_t.double() + bias.double()
    scale = cat.abs() @ w_t.double().abs() + bias.double().abs()
    agg_abs = torch.zeros_like(agg).index_add_(0, dst, x64[col.long()].abs()) / deg.clamp(min=1).double().unsqueeze(1)
    return (torch.relu(ref) if relu else ref), scale, agg, agg_abs


@pytest.mark.parametrize("F,N", [(100, 64), (128, 128), (256, 256)])
@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
def test_sage_layer_band_rows_at_three_extents(hiplib, far, precision, F, N):
    """The layer kernels' two addressing paths with live rows at the top of the extent: the largest table the 32-bit path takes
    (the last row below 2^31 bytes, read through buffer loads whose extent ends with it), the first 64-bit one (2^31 bytes), and
    the full view (offsets whose high word is 1, 2, 3 and 4; the fp32 kernel's 32-bit path ends at 2^32).  Forward and, for
    bf16x3, the training entry point that keeps the aggregate; int32 and int64 node lists and byte offsets."""
    import torch
    from wholegraph_amd import nn
    rows = fo.live_rows(F, 4)
    full = fo.view(far, F, torch.float32)
    vals_all = _values(len(rows), F, 31 * F + N)
    g = torch.Generator(device="cuda").manual_seed(F)
    w_t = torch.randn((2 * F, N), generator=g, device="cuda") * 0.2
    bias = torch.randn(N, generator=g, device="cuda")
    train = precision == "bf16x3" and nn.sage_layer_train_supported(F, N)
    assert train or precision == "f32"
    extents = list(fo.sage_extents(F))
    if precision == "f32":                       # its 32-bit path: x below 2^32 bytes
        extents += [((1 << 32) - 1) // (F * 4), -(-(1 << 32) // (F * 4))]
    with live(full, rows, vals_all):
        for x_rows in extents:
            keep = rows < x_rows
            assert rows[keep][-1] == x_rows - 1 or x_rows - 1 in rows, "no live row at the top of the extent"
            n_src = int(keep.sum())
            assert n_src >= 12
            vals = vals_all[:n_src].contiguous()
            x = fo.view(far, F, torch.float32, rows=x_rows)
            assert x.data_ptr() == far.data_ptr() and x.shape[0] == x_rows
            rp, col, self_rows = _hop(n_src, F + n_src)
            ar = torch.arange(n_src, device="cuda")

            def run(table, ids, relu=True):
                agg = torch.full((N_DST, F), 7.0, device="cuda") if train else None
                out = nn.sage_layer_fused_forward(rp, col, table, self_rows, w_t, bias, relu=relu, src_ids=ids,
                                                  precision=precision, agg_out=agg)
                return out, agg
            base, base_agg = run(vals, None)
            ref, scale, agg64, agg_abs = _sage_ref(rp, col, self_rows, vals, w_t, bias, True)
            _close(base, ref, scale, "%s F=%d x_rows=%d" % (precision, F, x_rows))
            got, got_agg = run(vals, ar)
            _same(got, base, "arange")
            forms = [("int32", x, _ids(rows[keep], torch.int32)), ("int64", x, _ids(rows[keep], torch.int64))]
            if precision == "bf16x3":
                forms.append(("byte offsets", nn.MappedTable(far.data_ptr(), F, far.device), _ids(rows[keep] * (F * 4), torch.int64)))
            for name, table, ids in forms:
                got, got_agg = run(table, ids)
                _same(got, base, "x_rows=%d %s" % (x_rows, name))
                if train:
                    _same(got_agg, base_agg, "x_rows=%d %s agg_out" % (x_rows, name))
            if train:
                _close(base_agg, agg64, agg_abs, "agg_out")
            fwd_only = nn.sage_layer_fused_forward(rp, col, x, self_rows, w_t, bias, relu=True, src_ids=forms[1][2], precision=precision)
            _same(fwd_only, base, "forward entry point")


# ---------------------------------------------------------------------------------------------------------------------
# sage_wgrad (wg_sage_bwd.hip)
# ---------------------------------------------------------------------------------------------------------------------
def _strided(far, n_rows, width, at=0):
    """float32 [n_rows, width] whose rows span the far buffer, starting ``at`` elements into it."""
    ld = fo.spanning_ld(n_rows, 1024)
    assert at + width <= 1024 and at % 4 == 0
    return fo.strided_view(far[at:], n_rows, width, ld)


@contextlib.contextmanager
def live_strided(v, values):
    import torch
    every = np.arange(v.shape[0])
    v[:] = values
    try:
        yield
    finally:
        fo.clear(v, every)
        assert fo.is_fill(v, every)


@pytest.mark.parametrize("F,N", [(100, 64), (128, 256)])
def test_sage_wgrad_band_rows_and_strided_operands(hiplib, far, F, N):
    """wgamd_sage_wgrad_bf16x3: the self rows through a node list into the far buffer (int32, int64, byte offsets), and —
    separately — agg, grad_out and act_out as strided views whose 333 rows span all four thresholds.  Deterministic (tests/
    test_gpu_sage_train.py): bit for bit the compact run; float64 at that file's bound."""
    import torch
    from wholegraph_amd import nn
    from test_gpu_sage_train import _close as close_train
    rows = fo.live_rows(F, 4)
    n_src = len(rows)
    v = fo.view(far, F, torch.float32)
    vals = _values(n_src, F, F + N)
    _, _, self_rows = _hop(n_src, N)
    agg, gout, act = _values(N_DST, F, 1), _values(N_DST, N, 2), _values(N_DST, N, 3)

    def run(x, ids, agg=agg, gout=gout, act=act):
        gwl, gwr, gb = torch.full((N, F), 7.0, device="cuda"), torch.full((N, F), 7.0, device="cuda"), torch.full((N,), 7.0, device="cuda")
        nn.sage_wgrad(agg, x, self_rows, gout, gwl, gwr, gb, act_out=act, src_ids=ids)
        return gwl, gwr, gb
    base = run(vals, None)
    dz = gout.double() * (act > 0)
    a64 = torch.cat([agg, vals[self_rows]], 1).double()
    ref, scale = dz.t() @ a64, dz.abs().t() @ a64.abs()
    close_train(base[0], ref[:, :F], scale[:, :F], "grad_w_l")
    close_train(base[1], ref[:, F:], scale[:, F:], "grad_w_r")
    close_train(base[2], dz.sum(0), dz.abs().sum(0), "grad_bias")
    for a, b in zip(run(vals, torch.arange(n_src, device="cuda")), base):
        _same(a, b, "arange")
    with live(v, rows, vals):
        forms = [("int32", v, _ids(rows, torch.int32)), ("int64", v, _ids(rows, torch.int64)),
                 ("byte offsets", nn.MappedTable(far.data_ptr(), F, far.device), _ids(rows * (F * 4), torch.int64))]
        for name, table, ids in forms:
            for a, b in zip(run(table, ids), base):
                _same(a, b, name)
    # the three row operands far apart: agg at column 0, grad_out at 256, act_out at 512 of every 1024-wide stride slot
    fa, fg, fc = _strided(far, N_DST, F, 0), _strided(far, N_DST, N, 256), _strided(far, N_DST, N, 512)
    with live_strided(fa, agg), live_strided(fg, gout), live_strided(fc, act):
        for a, b in zip(run(vals, None, fa, fg, fc), base):
            _same(a, b, "strided operands")


# ---------------------------------------------------------------------------------------------------------------------
# the x_row<KIND> layers: GCN, GIN, RGCN, TransformerConv, hetero SAGE
# ---------------------------------------------------------------------------------------------------------------------
def _forms(far, F, rows, vals, nn, byte_offsets=True):
    """[(name, table, ids, placement)]: id kinds 1, 2 and 3 into the far buffer and kind 0 through a strided x."""
    import torch
    v = fo.view(far, F, torch.float32)
    forms = [("int32", v, _ids(rows, torch.int32), lambda: live(v, rows, vals)),
             ("int64", v, _ids(rows, torch.int64), lambda: live(v, rows, vals))]
    if byte_offsets:
        forms.append(("byte offsets", nn.MappedTable(far.data_ptr(), F, far.device), _ids(rows * (F * 4), torch.int64),
                      lambda: live(v, rows, vals)))
    sx = fo.strided_view(far, len(rows), F, fo.spanning_ld(len(rows), F))
    forms.append(("strided x", sx, None, lambda: live_strided(sx, vals)))
    return forms


def _edges(rp):
    import torch
    deg = (rp[1:] - rp[:-1]).long()
    return torch.repeat_interleave(torch.arange(rp.shape[0] - 1, device="cuda"), deg)


def test_gcn_layer_aggregate_and_wgrad(hiplib, far):
    """gcn_layer (forward and _train), gcn_aggregate and gcn_wgrad (wg_gcn.hip), F = 64 -> N = 32, with edge weights, both
    normalisation vectors and added self loops, against gcn_ref.propagate in float64 at test_gpu_gcn.py's bound."""
    import torch
    from wholegraph_amd import nn
    from gcn_ref import propagate
    from test_gpu_gcn import _close as close_gcn
    F, N = 64, 32
    rows = fo.live_rows(F, 4)
    n_src = len(rows)
    vals = _values(n_src, F, 5)
    rp, col, self_rows = _hop(n_src, 6)
    E = col.shape[0]
    g = torch.Generator(device="cuda").manual_seed(7)
    ew = torch.rand(E, generator=g, device="cuda") + 0.25
    d_src = torch.rand(n_src, generator=g, device="cuda") + 0.5
    d_dst = torch.rand(N_DST, generator=g, device="cuda") + 0.5
    W = torch.randn((N, F), generator=g, device="cuda") * 0.2
    b = torch.randn(N, generator=g, device="cuda")
    fill = 2.0

    def run(x, ids):
        kw = dict(dinv_src=d_src, dinv_dst=d_dst, fill=fill, add_self_loops=True, src_ids=ids, edge_weight=ew)
        kept = torch.full((N_DST, F), 7.0, device="cuda")
        out = nn.gcn_layer_forward(rp, col, x, self_rows, W, b, relu=True, agg_out=kept, **kw)
        return out, kept, nn.gcn_layer_forward(rp, col, x, self_rows, W, b, relu=True, **kw), nn.gcn_aggregate(rp, col, x, self_rows, **kw)
    base = run(vals, None)
    _same(base[0], base[2], "train vs forward")
    _same(base[1], base[3], "kept aggregate vs aggregate kernel")
    # float64: loop edges (col == the row's self row) are not summed, the last one gives the added loop its weight
    dst = _edges(rp)
    loop = col.long() == self_rows[dst]
    loopw = np.full(N_DST, fill)
    for e in torch.nonzero(loop).flatten().tolist():
        loopw[int(dst[e])] = float(ew[e])
    loopw = torch.from_numpy(loopw).cuda()
    coef = (ew.double() * d_src.double()[col.long()] * d_dst.double()[dst])[~loop]
    x64 = vals.double()
    self_term = (loopw * d_src.double()[self_rows] * d_dst.double()).unsqueeze(1)
    agg64 = propagate(col.long()[~loop], dst[~loop], coef, x64, N_DST) + self_term * x64[self_rows]
    agg_abs = propagate(col.long()[~loop], dst[~loop], coef, x64.abs(), N_DST) + self_term * x64[self_rows].abs()
    close_gcn(base[3], agg64, agg_abs, "aggregate")
    close_gcn(base[0], torch.relu(agg64 @ W.double().t() + b.double()), agg_abs @ W.double().abs().t() + b.double().abs(), "layer")
    for a, c in zip(run(vals, torch.arange(n_src, device="cuda")), base):
        _same(a, c, "arange")
    for name, table, ids, placed in _forms(far, F, rows, vals, nn):
        with placed():
            for a, c in zip(run(table, ids), base):
                _same(a, c, name)
    # the weight gradient over strided far operands
    gout, act = _values(N_DST, N, 8), base[0]

    def wgrad(agg, gout, act):
        gw, gb = torch.full((N, F), 7.0, device="cuda"), torch.full((N,), 7.0, device="cuda")
        nn.gcn_wgrad(agg, gout, gw, gb, act_out=act)
        return gw, gb
    gw, gb = wgrad(base[1], gout, act)
    dz = gout.double() * (act > 0)
    close_gcn(gw, dz.t() @ base[1].double(), dz.abs().t() @ base[1].double().abs(), "dW")
    close_gcn(gb, dz.sum(0), dz.abs().sum(0), "db")
    fa, fg, fc = _strided(far, N_DST, F, 0), _strided(far, N_DST, N, 256), _strided(far, N_DST, N, 512)
    with live_strided(fa, base[1]), live_strided(fg, gout), live_strided(fc, act):
        for a, c in zip(wgrad(fa, fg, fc), (gw, gb)):
            _same(a, c, "wgrad over strided operands")


def test_gin_layer_and_aggregate(hiplib, far):
    """gin_layer (two products, F = 64 -> 64 -> 32) and gin_aggregate (wg_gin.hip) against gin_ref at test_gpu_gin.py's bound."""
    import torch
    from wholegraph_amd import nn
    import gin_ref
    from test_gpu_gin import _close as close_gin
    F, H, N = 64, 64, 32
    assert nn.gin_layer_supported(F, H, N)
    rows = fo.live_rows(F, 4)
    n_src = len(rows)
    vals = _values(n_src, F, 15)
    rp, col, self_rows = _hop(n_src, 16)
    g = torch.Generator(device="cuda").manual_seed(17)
    w1, b1 = torch.randn((H, F), generator=g, device="cuda") * 0.2, torch.randn(H, generator=g, device="cuda")
    w2, b2 = torch.randn((N, H), generator=g, device="cuda") * 0.2, torch.randn(N, generator=g, device="cuda")
    eps = torch.tensor([0.25], device="cuda")

    def run(x, ids):
        return (nn.gin_layer_forward(rp, col, x, self_rows, w1, b1, w2, b2, eps=eps, relu_out=True, src_ids=ids),
                nn.gin_aggregate(rp, col, x, self_rows, eps=eps, src_ids=ids))
    base = run(vals, None)
    ei = torch.stack([col.long(), _edges(rp)])
    kw = dict(eps=0.25, x_dst=vals[self_rows], num_dst=N_DST)
    close_gin(base[1], gin_ref.gin_aggregate(vals, ei, **kw), gin_ref.gin_aggregate(vals, ei, abs_terms=True, **kw), "aggregate")
    close_gin(base[0], gin_ref.gin_forward(vals, ei, w1, b1, w2, b2, relu=True, **kw),
              gin_ref.gin_forward(vals, ei, w1, b1, w2, b2, abs_terms=True, **kw), "layer")
    for a, c in zip(run(vals, torch.arange(n_src, device="cuda")), base):
        _same(a, c, "arange")
    for name, table, ids, placed in _forms(far, F, rows, vals, nn):
        with placed():
            for a, c in zip(run(table, ids), base):
                _same(a, c, name)


def test_rgcn_layer_and_wgrad(hiplib, far):
    """rgcn_layer_forward and rgcn_wgrad (wg_rgcn.hip), three relations, F = 64 -> N = 32 with a root term, against rgcn_ref
    over the hop's bipartite graph (destination i = node n_src + i, whose row is x[self_rows[i]])."""
    import torch
    from wholegraph_amd import nn
    import rgcn_ref
    from test_gpu_rgcn import _close as close_rgcn
    F, N, R = 64, 32, 3
    assert nn.rgcn_layer_supported(F, N, R, True)
    rows = fo.live_rows(F, 4)
    n_src = len(rows)
    vals = _values(n_src, F, 25)
    rp, col, self_rows = _hop(n_src, 26)
    E = col.shape[0]
    g = torch.Generator(device="cuda").manual_seed(27)
    et = torch.randint(0, R, (E,), generator=g, device="cuda")
    weight = torch.randn((R, F, N), generator=g, device="cuda") * 0.2
    root = torch.randn((F, N), generator=g, device="cuda") * 0.2
    bias = torch.randn(N, generator=g, device="cuda")
    rel, coef = nn.rgcn_edge_coef(rp, et, R, mean=True)
    wt = torch.cat([weight[r] for r in range(R)] + [root], 0).t().contiguous()          # [N, (R + 1) F]
    dst = _edges(rp)
    gout = _values(N_DST, N, 28)
    seg = rel.long()

    def run(x, ids):
        out = nn.rgcn_layer_forward(rp, col, x, self_rows, rel, coef, wt, None, R, True, bias=bias, relu=True, src_ids=ids)
        return out, nn.rgcn_wgrad(x, col.long(), dst, coef, seg, R, gout, src_ids=ids)
    base = run(vals, None)
    x_ext = torch.cat([vals, vals[self_rows]], 0)
    ei = torch.stack([col.long(), n_src + dst])
    kw = dict(root=root, bias=bias, aggr="mean", num_relations=R)
    close_rgcn(base[0], rgcn_ref.rgcn_forward(x_ext, ei, et, weight, relu=True, **kw)[n_src:],
               rgcn_ref.rgcn_forward(x_ext, ei, et, weight, abs_terms=True, **kw)[n_src:], "layer")
    x64, c64, g64 = vals.double()[col.long()], coef.double().unsqueeze(1), gout.double()[dst]
    for r in range(R):
        m = seg == r
        close_rgcn(base[1][r], (c64[m] * x64[m]).t() @ g64[m], (c64[m] * x64[m]).abs().t() @ g64[m].abs(), "wgrad %d" % r)
    for a, c in zip(run(vals, torch.arange(n_src, device="cuda")), base):
        _same(a, c, "arange")
    for name, table, ids, placed in _forms(far, F, rows, vals, nn):
        with placed():
            for a, c in zip(run(table, ids), base):
                _same(a, c, name)


def test_transformer_layer_forward_and_backward(hiplib, far):
    """TransformerConv on the one-kernel route (transformer_layer_forward, transformer_bwd_dst, transformer_bwd_src; wg_
    transformer.hip), H = 2 x C = 16 over F = 64, x read through LazyRows of every id kind and as a strided tensor: output,
    attention weights and every parameter gradient bit for bit the compact run's; output and gradients against the float64
    restatement at test_gpu_transformer.py's bounds."""
    import torch
    from wholegraph_amd import nn
    from transformer_ref import params_of, transformer_forward
    from test_gpu_transformer import _close as close_t, _close_grad, _conv
    F, C, H = 64, 16, 2
    rows = fo.live_rows(F, 4, per_band=44)          # 378 input rows: every destination has an input row of its own
    n_src = len(rows)
    vals = _values(n_src, F, 35)
    rp, col, self_rows = _hop(n_src, 36, distinct_self_rows=True)
    conv = _conv(F, C, H, True, None, seed=37)
    lg = nn.LayerGraph([nn.HopGraph(rp, col, self_rows)])
    G = _values(N_DST, H * C, 38)
    calls = []
    orig = (nn.transformer_layer_forward, nn.transformer_bwd_dst, nn.transformer_bwd_src)

    def run(x):
        conv.zero_grad(set_to_none=True)
        out, alpha = conv(x, lg, act="relu", return_attention_weights=True)
        (out * G).sum().backward()
        grads = {k: p.grad.clone() for k, p in conv.named_parameters()}
        xg = x.grad.clone() if torch.is_tensor(x) and x.grad is not None else None
        return out.detach().clone(), alpha.clone(), grads, xg
    try:      # count the launches: every run must take the kernel route, forward and both backward launches
        nn.transformer_layer_forward = lambda *a, **k: calls.append("fwd") or orig[0](*a, **k)
        nn.transformer_bwd_dst = lambda *a, **k: calls.append("dst") or orig[1](*a, **k)
        nn.transformer_bwd_src = lambda *a, **k: calls.append("src") or orig[2](*a, **k)
        base = run(vals.clone().requires_grad_(True))
        assert calls[0] == "fwd" and sorted(calls) == ["dst", "fwd", "src"], calls
        p64 = {k: None if t is None else t.double().requires_grad_(True) for k, t in params_of(conv).items()}
        x64 = vals.double().requires_grad_(True)
        ei = torch.stack([col.long(), _edges(rp)])
        ref = transformer_forward(x64, x64[self_rows], ei, p64, H, True, None, relu=True)
        scale = transformer_forward(x64.detach(), x64.detach()[self_rows], ei, params_of(conv), H, True, None, abs_terms=True)
        close_t(base[0], ref.detach(), scale, "forward")
        (ref * G.double()).sum().backward()
        names = {"lin_query.weight": "Wq", "lin_query.bias": "bq", "lin_key.weight": "Wk", "lin_value.weight": "Wv",
                 "lin_value.bias": "bv", "lin_skip.weight": "Ws", "lin_skip.bias": "bs"}
        for k, r in names.items():
            if k in base[2]:
                _close_grad(base[2][k], p64[r].grad, "d" + k)
        _close_grad(base[3], x64.grad, "dx")
        lazy = [("arange", lambda: nn.LazyRows(vals, torch.arange(n_src, device="cuda")), contextlib.nullcontext)]
        for name, table, ids, placed in _forms(far, F, rows, vals, nn):
            if ids is None:
                lazy.append((name, (lambda t=table: t.requires_grad_(False)), placed))
            else:
                def make(t=table, i=ids):
                    rows_ = nn.LazyRows(t, i)
                    if isinstance(t, nn.MappedTable):
                        rows_._gather = lambda: vals
                    return rows_
                lazy.append((name, make, placed))
        for name, make, placed in lazy:
            del calls[:]
            with placed():
                got = run(make())
            assert calls[0] == "fwd" and "dst" in calls, (name, calls)
            _same(got[0], base[0], name + " out")
            _same(got[1], base[1], name + " alpha")
            for k in base[2]:
                _same(got[2][k], base[2][k], name + " d" + k)
    finally:
        nn.transformer_layer_forward, nn.transformer_bwd_dst, nn.transformer_bwd_src = orig


def test_hetero_sage_layer(hiplib, far):
    """wgamd_hetero_sage_layer_f32 (wg_sage_hetero.hip): two relations of different widths ending in one type, both read through
    node lists into the far buffer (kinds 1 and 2; the entry point has no byte-offset kind), the root rows through a list as
    well — against hetero_sage_ref at test_gpu_hetero_sage.py's bound."""
    import types
    import torch
    from wholegraph_amd import nn
    from hetero_sage_ref import hetero_sage_forward
    Fa, Fb, N = 64, 32, 32
    rows_a, rows_b = fo.live_rows(Fa, 4), fo.live_rows(Fb, 4)
    va, vb = _values(len(rows_a), Fa, 45), _values(len(rows_b), Fb, 46)
    rpa, cola, dst_rows = _hop(len(rows_a), 47)
    rpb, colb, _ = _hop(len(rows_b), 48)
    g = torch.Generator(device="cuda").manual_seed(49)
    Wla, Wlb = torch.randn((N, Fa), generator=g, device="cuda") * 0.2, torch.randn((N, Fb), generator=g, device="cuda") * 0.2
    Wra, Wrb = torch.randn((N, Fa), generator=g, device="cuda") * 0.2, torch.randn((N, Fa), generator=g, device="cuda") * 0.2
    bla, blb = torch.randn(N, generator=g, device="cuda"), torch.randn(N, generator=g, device="cuda")
    wt = torch.cat([Wla, Wlb, Wra + Wrb], 1).contiguous()
    bias = bla + blb
    ea, eb = ("a", "to", "a"), ("b", "to", "a")

    def run(xa, ida, xb, idb):
        rels = [(rpa, cola, xa, ida, None, True), (rpb, colb, xb, idb, None, False)]
        return nn.hetero_sage_launch(rels, N_DST, wt, N, root=(xa, dst_rows, ida), bias=bias, relu=True)
    base = run(va, None, vb, None)
    rel = lambda et, rp, col: types.SimpleNamespace(hop=0, edge_type=et, n_rows=N_DST, row_ptr=rp, col=col, n_edges=int(col.shape[0]),  # noqa: E731
                                                    dst_rows=dst_rows, out_rows=None)
    graph = types.SimpleNamespace(relations=[rel(ea, rpa, cola), rel(eb, rpb, colb)], n_out={"a": N_DST})
    params = {ea: dict(Wl=Wla, bl=bla, Wr=Wra, mean=True), eb: dict(Wl=Wlb, bl=blb, Wr=Wrb, mean=False)}
    xs = {"a": va, "b": vb}
    err = (base.double() - hetero_sage_forward(xs, graph, params, relu=True)["a"]).abs()
    mag = hetero_sage_forward(xs, graph, params, abs_terms=True)["a"]
    print("hetero layer max err / bound %.3f" % float((err / (1e-5 * mag)).max()))
    assert bool(torch.isfinite(base).all()) and bool((err <= 1e-5 * mag).all()), float(err.max())     # (test_gpu_hetero_sage.py's bar)
    ar = lambda n: torch.arange(n, device="cuda")  # noqa: E731
    _same(run(va, ar(len(rows_a)), vb, ar(len(rows_b))), base, "arange")
    fa, fb = fo.view(far, Fa, torch.float32), fo.view(far, Fb, torch.float32)
    # both views start at the buffer's first byte and their bands meet at every threshold: one relation's table at a time
    with live(fa, rows_a, va):
        for dt in (torch.int32, torch.int64):
            _same(run(fa, _ids(rows_a, dt), vb, None), base, "relation a %s" % dt)
    with live(fb, rows_b, vb):
        for dt in (torch.int32, torch.int64):
            _same(run(va, None, fb, _ids(rows_b, dt)), base, "relation b %s" % dt)
    sx = fo.strided_view(far, len(rows_a), Fa, fo.spanning_ld(len(rows_a), Fa))
    with live_strided(sx, va):
        _same(run(sx, None, vb, None), base, "strided x")


def test_hetero_transformer_layer(hiplib, far):
    """wgamd_hetero_transformer_layer_f32(_train) (wg_transformer_hetero.hip): two relations (H = 2 with edge attributes over F = 64,
    H = 1 over F = 32) ending in one type, both read through node lists into the far buffer (kinds 1 and 2), the root rows through
    a list as well, and ``out`` at band rows of a far view through ``out_rows``: output, kept A and every alpha bit for bit the
    compact run's — which is within test_gpu_hetero_transformer.py's bound of the float64 restatement."""
    import torch
    from wholegraph_amd import nn
    from hetero_launch_ref import block_width, hetero_transformer_launch_ref
    Fa, Fb, Ha, Hb, D, N = 64, 32, 2, 1, 3, 32
    rows_a, rows_b = fo.live_rows(Fa, 4), fo.live_rows(Fb, 4)
    va, vb = _values(len(rows_a), Fa, 75), _values(len(rows_b), Fb, 76)
    rpa, cola, dst_rows = _hop(len(rows_a), 77)
    rpb, colb, _ = _hop(len(rows_b), 78)
    g = torch.Generator(device="cuda").manual_seed(79)
    rnd = lambda *s: torch.randn(s, generator=g, device="cuda")  # noqa: E731
    ea = rnd(int(cola.shape[0]), D)
    ua, wa, ub = rnd(N_DST, Ha * Fa) * 0.2, rnd(N_DST, Ha * D) * 0.5, rnd(N_DST, Hb * Fb) * 0.3
    K = Ha * block_width(Fa, D) + Hb * block_width(Fb, 0) + Fa
    wt, bias = rnd(N, K) * 0.2, rnd(N)

    def run(xa, ida, xb, idb, out=None, out_rows=None):
        A = torch.empty((N_DST, K), device="cuda")
        al = [torch.empty((int(cola.shape[0]), Ha), device="cuda"), torch.empty((int(colb.shape[0]), Hb), device="cuda")]
        rels = [(rpa, cola, xa, ida, ea, ua, wa, Ha, al[0]), (rpb, colb, xb, idb, None, ub, None, Hb, al[1])]
        before = nn.hetero_transformer_launches
        out = nn.hetero_transformer_launch(rels, N_DST, wt, N, root=(xa, dst_rows, ida), bias=bias, relu=True, out_rows=out_rows,
                                           out=out, a_save=A)
        assert nn.hetero_transformer_launches - before == 1
        return out, A, al[0], al[1]

    def same(got, what):
        for a, c, part in zip(got, base, ("out", "A", "alpha a", "alpha b")):
            _same(a, c, "%s %s" % (what, part))
    base = run(va, None, vb, None)
    rels64 = [(rpa, cola, va, None, ea, ua, wa, Ha, None), (rpb, colb, vb, None, None, ub, None, Hb, None)]
    ref, _, mag, ralpha = hetero_transformer_launch_ref(rels64, N_DST, wt, N, root=(va, dst_rows, None), bias=bias, relu=True)
    err = (base[0].double() - ref).abs()
    print("hetero transformer layer max err / bound %.3f" % float((err / (1e-5 * mag)).max()))
    assert bool(torch.isfinite(base[0]).all()) and bool((err <= 1e-5 * mag).all()), float(err.max())   # (test_gpu_hetero_transformer.py's bar)
    assert all(float((a.double() - b).abs().max()) <= 1e-5 for a, b in zip(base[2:], ralpha))
    ar = lambda n: torch.arange(n, device="cuda")  # noqa: E731
    same(run(va, ar(len(rows_a)), vb, ar(len(rows_b))), "arange")
    fa, fb = fo.view(far, Fa, torch.float32), fo.view(far, Fb, torch.float32)
    # both views start at the buffer's first byte and their bands meet at every threshold: one relation's table at a time
    with live(fa, rows_a, va):
        for dt in (torch.int32, torch.int64):
            same(run(fa, _ids(rows_a, dt), vb, None), "relation a %s" % dt)
    with live(fb, rows_b, vb):
        for dt in (torch.int32, torch.int64):
            same(run(va, None, fb, _ids(rows_b, dt)), "relation b %s" % dt)
    sx = fo.strided_view(far, len(rows_a), Fa, fo.spanning_ld(len(rows_a), Fa))
    with live_strided(sx, va):
        same(run(sx, None, vb, None), "strided x")
    # out_rows: band row numbers of a [rows, N] view of the far buffer (as test_far_outputs_of_the_sage_and_gcn_layers)
    v = fo.view(far, N, torch.float32)
    rows = fo.live_rows(N, 4, per_band=44)
    rows = np.concatenate([rows[:N_DST - 1], rows[-1:]])
    assert len(rows) == N_DST and rows[-1] == v.shape[0] - 1
    out_rows = torch.from_numpy(rows).cuda()
    try:
        got = run(va, None, vb, None, out=v, out_rows=out_rows)
        torch.cuda.synchronize()
        same((v[out_rows],) + got[1:], "out_rows")
        assert fo.is_fill(v, fo.neighbours(rows, v.shape[0]))
    finally:
        fo.clear(v, rows)


# ---------------------------------------------------------------------------------------------------------------------
# GAT (forward)
# ---------------------------------------------------------------------------------------------------------------------
def test_gat_aggregate_and_fused_layer(oracle_mod, hiplib, far):
    """gat_aggregate_heads and gat_layer_fused with src_ids (int64: the only kind they take), F = 128, 4 heads x 64, against the
    oracle's aggregate and its float64 one times the weight (tests/test_gpu_mag_pipeline.py's bounds)."""
    import torch
    from wholegraph_amd import nn
    F, H, C = 128, 4, 64
    assert nn.gat_layer_fused_supported(F, H, C)
    rows = fo.live_rows(F, 4)
    n_src = len(rows)
    vals = _values(n_src, F, 55)
    rp, col, dst_rows = _hop(n_src, 56)
    g = torch.Generator(device="cuda").manual_seed(57)
    a_src = torch.randn((n_src, H), generator=g, device="cuda") * 2
    a_dst = torch.randn((n_src, H), generator=g, device="cuda") * 2
    w = torch.randn((F, H * C), generator=g, device="cuda") / F ** 0.5
    bias = torch.randn(H * C, generator=g, device="cuda")

    def run(x, ids):
        return (nn.gat_aggregate_heads(rp, col, x, a_src, a_dst, H, dst_rows=dst_rows, src_ids=ids),
                nn.gat_layer_fused(rp, col, x, a_src, a_dst, w, H, dst_rows=dst_rows, bias=bias, relu=True, src_ids=ids))
    base = run(vals, None)
    cpu = lambda t: t.cpu().numpy()  # noqa: E731
    ref = oracle_mod.gat_aggregate_heads(cpu(rp), cpu(col), cpu(vals), cpu(a_src), cpu(a_dst), dst_rows=cpu(dst_rows))
    np.testing.assert_allclose(cpu(base[0]).reshape(N_DST, H, F), ref, rtol=1e-5, atol=2e-6)
    agg64 = oracle_mod.gat_aggregate_heads_f64(cpu(rp), cpu(col), cpu(vals).astype(np.float64), cpu(a_src), cpu(a_dst), dst_rows=cpu(dst_rows))
    abs64 = oracle_mod.gat_aggregate_heads_f64(cpu(rp), cpu(col), np.abs(cpu(vals)).astype(np.float64), cpu(a_src), cpu(a_dst), dst_rows=cpu(dst_rows))
    w64 = cpu(w).astype(np.float64).reshape(F, H, C)
    want = np.maximum(np.einsum("nhf,fhc->nhc", agg64, w64).reshape(N_DST, H * C) + cpu(bias), 0)
    scale = np.einsum("nhf,fhc->nhc", abs64, np.abs(w64)).reshape(N_DST, H * C) + np.abs(cpu(bias))
    err = np.abs(cpu(base[1]) - want)
    print("gat layer max err / bound %.3f" % (err / (1e-5 * scale + 1e-7)).max())
    assert np.all(err <= 1e-5 * scale + 1e-7), err.max()
    for a, c in zip(run(vals, torch.arange(n_src, device="cuda")), base):
        _same(a, c, "arange")
    v = fo.view(far, F, torch.float32)
    with live(v, rows, vals):
        for a, c in zip(run(v, _ids(rows, torch.int64)), base):
            _same(a, c, "int64")


# ---------------------------------------------------------------------------------------------------------------------
# far outputs
# ---------------------------------------------------------------------------------------------------------------------
def test_far_outputs_of_the_sage_and_gcn_layers(hiplib, far):
    """``out`` (and the kept aggregate) as strided views of the far buffer whose 333 rows cross all four thresholds, for the
    bf16x3 SAGE layer and for GCN (a ``launch_tiles`` layer), and the hetero SAGE layer's ``out_rows`` with band row numbers and
    a normal row stride: read back with torch, equal to the compact run, every row in between still NaN."""
    import torch
    from wholegraph_amd import nn
    F, N = 128, 64
    n_src = 80
    vals = _values(n_src, F, 65)
    rp, col, self_rows = _hop(n_src, 66)
    g = torch.Generator(device="cuda").manual_seed(67)
    w_t = torch.randn((2 * F, N), generator=g, device="cuda") * 0.2
    W = torch.randn((N, F), generator=g, device="cuda") * 0.2
    bias = torch.randn(N, generator=g, device="cuda")
    every = np.arange(N_DST)
    out_far, agg_far = _strided(far, N_DST, N, 0), _strided(far, N_DST, F, 256)
    between = fo.strided_view(far[out_far.stride(0) // 2:], N_DST - 1, 1024, out_far.stride(0))     # half a stride further on
    cases = {
        "sage": lambda out, agg: nn.sage_layer_fused_forward(rp, col, vals, self_rows, w_t, bias, relu=True, precision="bf16x3",
                                                             out=out, agg_out=agg),
        "gcn": lambda out, agg: nn.gcn_layer_forward(rp, col, vals, self_rows, W, bias, relu=True, out=out, agg_out=agg),
    }
    for name, launch in cases.items():
        want, want_agg = torch.empty((N_DST, N), device="cuda"), torch.empty((N_DST, F), device="cuda")
        launch(want, want_agg)
        try:
            got = launch(out_far, agg_far)
            torch.cuda.synchronize()
            assert got.data_ptr() == far.data_ptr()
            _same(out_far.clone(), want, name + " out")
            _same(agg_far.clone(), want_agg, name + " kept aggregate")
            assert fo.is_fill(between, every[:-1]), name + ": wrote between its output rows"
            assert bool(torch.isnan(far[N:256]).all()) and bool(torch.isnan(far[256 + F:out_far.stride(0)]).all())
        finally:
            fo.clear(out_far, every)
            fo.clear(agg_far, every)
    # out_rows: band row numbers of a [rows, N] view, normal row stride (the hetero SAGE layer's row placement)
    v = fo.view(far, N, torch.float32)
    rows = fo.live_rows(N, 4, per_band=44)[:N_DST + 40]
    rows = np.concatenate([rows[:N_DST - 1], fo.live_rows(N, 4, per_band=44)[-1:]])
    assert len(rows) == N_DST and rows[-1] == v.shape[0] - 1
    out_rows = torch.from_numpy(rows).cuda()
    wt = torch.cat([W, W * 0.5], 1).contiguous()
    rels = [(rp, col, vals, None, None, True)]
    want = nn.hetero_sage_launch(rels, N_DST, wt, N, root=(vals, self_rows, None), bias=bias, relu=True)
    try:
        nn.hetero_sage_launch(rels, N_DST, wt, N, root=(vals, self_rows, None), bias=bias, relu=True, out_rows=out_rows, out=v)
        torch.cuda.synchronize()
        _same(v[out_rows], want, "out_rows")
        assert fo.is_fill(v, fo.neighbours(rows, v.shape[0]))
    finally:
        fo.clear(v, rows)


# ---------------------------------------------------------------------------------------------------------------------
# sampling (wg_sample.hip, wg_sample_replace.hip, wg_fused.hip)
# ---------------------------------------------------------------------------------------------------------------------
V_SAMPLE = 4000


def _far_csr(n_entries, centers, seed, max_deg=200):
    """A CSR of 4,000 vertices in compact form and spread over ``n_entries`` col entries: ``len(centers) + 1`` giant vertices that no
    col entry names (degree 0 in the compact form) push the bands of real rows between them to straddle the edge indices
    ``centers`` (the last band ends with the last entry of the view).  -> (row_ptr, row_ptr_far, col, bands, giants, shift) with
    ``bands`` = [(compact start, far start, length)] and ``shift[v]`` = far - compact position of row v's edges."""
    rng = np.random.default_rng(seed)
    V = V_SAMPLE
    n_bands = len(centers) + 2                                            # one at entry 0, one per centre, one at the top
    giants = [(k + 1) * V // n_bands for k in range(n_bands - 1)]
    real = np.setdiff1d(np.arange(V), giants)
    deg = rng.integers(0, max_deg + 1, V)
    deg[rng.permutation(real)[:120]] = np.repeat([0, 4, 5, 6, 24, 25, 26, 39, 40, 41], 12)
    for gv in giants:                       # real rows directly before and after every giant row
        deg[gv - 1], deg[gv + 1] = 30, 7
    deg[giants] = 0
    rp = np.zeros(V + 1, np.int64)
    rp[1:] = np.cumsum(deg)
    col = real[rng.integers(0, len(real), rp[-1])]
    edges = [0] + [int(rp[gv]) for gv in giants] + [int(rp[-1])]          # compact edge range of every band
    bands, shift = [], np.zeros(V + 1, np.int64)
    for k in range(n_bands):
        a, n = edges[k], edges[k + 1] - edges[k]
        s = 0 if k == 0 else (n_entries - n if k == n_bands - 1 else centers[k - 1] - n // 2)
        assert k in (0, n_bands - 1) or s < centers[k - 1] < s + n
        bands.append((a, s, n))
        first = 0 if k == 0 else giants[k - 1] + 1
        last = giants[k] if k < n_bands - 1 else V
        shift[first:last + 1] = s - a
        assert k == 0 or s > bands[k - 1][1] + bands[k - 1][2], "bands overlap"
    rp_far = rp + shift
    assert rp_far[-1] == n_entries and np.all(np.diff(rp_far) >= 0)
    assert all(rp_far[gv + 1] - rp_far[gv] > 1 << 26 for gv in giants) and not np.isin(col, giants).any()
    return rp, rp_far, col, bands, giants, shift


def _far_graph(far, col_dtype, seed):
    """``_far_csr`` for a col array that is the far buffer seen as ``col_dtype``; centers at byte 2^31 and 2^32 and at entries
    2^30 and 2^31 (int32: the top band lies at entry 2^32; int64: it straddles 2^31).  The real rows' entries are written, the
    rest stays NaN bits (2143289344 as int32: no vertex)."""
    import torch
    tdt = getattr(torch, col_dtype)
    col_far = fo.flat_view(far, tdt)
    elem = col_far.element_size()
    centers = sorted({(1 << 31) // elem, (1 << 32) // elem, 1 << 30, 1 << 31} - ({1 << 31} if elem == 8 else set()))
    rp, rp_far, col, bands, giants, shift = _far_csr(col_far.numel(), centers, seed)
    top = bands[-1]
    assert top[1] + top[2] == col_far.numel() and top[1] < (1 << 32 if elem == 4 else 1 << 31) < top[1] + top[2]
    assert rp_far[-1] > (1 << 32 if elem == 4 else 1 << 31)
    return rp, rp_far, col.astype(col_dtype), bands, giants, shift, col_far


@contextlib.contextmanager
def live_col(col_far, bands, col):
    import torch
    t = torch.from_numpy(col).cuda()
    for a, s, n in bands:
        col_far[s:s + n] = t[a:a + n]
    try:
        yield
    finally:
        for a, s, n in bands:
            fo.clear_span(col_far, s, s + n)


def _sample_seeds(giants, seed, n, dtype):
    rng = np.random.default_rng(seed)
    real = np.setdiff1d(np.arange(V_SAMPLE), giants)
    near = np.array([gv + d for gv in giants for d in (-2, -1, 1, 2)] + [0, V_SAMPLE - 1])
    return np.concatenate([near, rng.choice(real, n - len(near))]).astype(dtype)


@pytest.mark.parametrize("col_dtype", ["int32", "int64"])
def test_uniform_hops_over_a_far_col_array(oracle_mod, hiplib, far, col_dtype):
    """wholegraph_csr_unweighted_sample_without_replacement with fan-outs 5 and 25 (rows shorter than, as long as and longer than
    the fan-out: the copy and half-wave kernels), 40 (the block kernel) and sample-all, and the with-replacement hop: offsets,
    neighbours and local ids bit for bit the compact graph's (itself bit for bit the oracle's, as tests/test_gpu_sampling.py
    has it), edge ids equal after subtracting each row's shift — ids beyond 2^31 and 2^32 come out whole."""
    import torch
    from wholegraph_amd import wholegraph_ops as ops
    from test_gpu_sampling import _run
    rp, rp_far, col, bands, giants, shift, col_far = _far_graph(far, col_dtype, 1)
    rpf = torch.from_numpy(rp_far).cuda()
    with live_col(col_far, bands, col):
        for M, seed_dtype in ((5, np.int64), (25, np.int32), (40, np.int64), (-1, np.int64)):
            seeds = _sample_seeds(giants, M + 100, 600, seed_dtype)
            want = [t.cpu().numpy() for t in _run(oracle_mod, rp, col, seeds, M, 777 + M)]
            got = [t.cpu().numpy() for t in ops.unweighted_sample_without_replacement(
                rpf, col_far, torch.from_numpy(seeds).cuda(), M, random_seed=777 + M, need_center_local_output=True, need_edge_output=True)]
            _same_sample(got, want, seeds, shift, "M=%d" % M)
            assert got[3].max() > (1 << 32 if col_dtype == "int32" else 1 << 31)
        for M in (5, 25):
            seeds = _sample_seeds(giants, M + 200, 600, np.int64)
            want = [t.cpu().numpy() for t in ops.unweighted_sample_with_replacement(
                torch.from_numpy(rp).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(seeds).cuda(), M, random_seed=55 + M,
                need_center_local_output=True, need_edge_output=True)]
            ref = oracle_mod.unweighted_sample_with_replacement(rp, col, seeds, M, 55 + M)
            assert all(np.array_equal(a, b) for a, b in zip(want, ref))
            got = [t.cpu().numpy() for t in ops.unweighted_sample_with_replacement(
                rpf, col_far, torch.from_numpy(seeds).cuda(), M, random_seed=55 + M, need_center_local_output=True, need_edge_output=True)]
            _same_sample(got, want, seeds, shift, "with replacement M=%d" % M)


def _same_sample(got, want, seeds, shift, what):
    for name, a, b in zip(("offsets", "neighbours", "local ids"), got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b), "%s: %s differ at %s" % (what, name, np.nonzero(a != b)[0][:8])
    gid = got[3] - shift[seeds[got[2]]]
    assert np.array_equal(gid, want[3]), "%s: edge ids differ at %s" % (what, np.nonzero(gid != want[3])[0][:8])


@pytest.mark.parametrize("col_dtype", ["int32", "int64"])
def test_call_group_and_pyg_hops_over_a_far_col_array(hiplib, far, col_dtype):
    """The batched call-group hop (NoSyncWalk, two hops of fan-outs 10 and 5 over 4 batches) and the PyG hop (PygNoSyncWalk, fan-
    outs 5 and 25, with edge ids) read the far col array directly (no 32-bit twin): every live output equals the compact
    graph's, PyG's edge ids after subtracting each row's shift."""
    import torch
    from wholegraph_amd.fused import NoSyncWalk, PygNoSyncWalk
    rp, rp_far, col, bands, giants, shift, col_far = _far_graph(far, col_dtype, 2)
    tdt = getattr(torch, col_dtype)
    G, B = 4, 64
    seeds = torch.from_numpy(_sample_seeds(giants, 9, G * B, col_dtype)).cuda()
    rpc, colc, rpf = torch.from_numpy(rp).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(rp_far).cuda()
    rs = [[11, 12, 13, 14], [21, 22, 23, 24]]
    with live_col(col_far, bands, col):
        a = NoSyncWalk(rpc, colc, B, [10, 5], id_dtype=tdt, n_batches=G, compact_col=False).run(seeds, rs)
        b = NoSyncWalk(rpf, col_far, B, [10, 5], id_dtype=tdt, n_batches=G, compact_col=False).run(seeds, rs)
        torch.cuda.synchronize()
        _same(b.counts, a.counts, "counts")
        n_targets = G * B
        for k in range(2):
            e, u = (int(c) for c in a.counts[k])
            assert e > 0 and u > 0
            _same(b.offsets[k][:n_targets + 1], a.offsets[k][:n_targets + 1], "hop %d offsets" % k)
            _same(b.neighbor_row[k][:e], a.neighbor_row[k][:e], "hop %d neighbour rows" % k)
            _same(b.center_row[k][:e], a.center_row[k][:e], "hop %d centre rows" % k)
            _same(b.unique[k][:u], a.unique[k][:u], "hop %d node list" % k)
            _same(b.unique_seg[k], a.unique_seg[k], "hop %d segments" % k)
            n_targets = u
        shift_t = torch.from_numpy(shift).cuda()
        pa = PygNoSyncWalk(rpc, colc, B, [5, 25], n_batches=G, compact_col=False).run(seeds, rs).finalize_batches()
        pb = PygNoSyncWalk(rpf, col_far, B, [5, 25], n_batches=G, compact_col=False).run(seeds, rs).finalize_batches()
        far_ids = 0
        for (node_a, row_a, col_a, edge_a, nn_a, ne_a), (node_b, row_b, col_b, edge_b, nn_b, ne_b) in zip(pa, pb):
            _same(node_b, node_a, "nodes")
            _same(row_b, row_a, "rows")
            _same(col_b, col_a, "cols")
            assert nn_a == nn_b and ne_a == ne_b
            owner = torch.searchsorted(rpf, edge_b, right=True) - 1            # the row an edge id lies in
            assert not bool(torch.isin(owner, torch.tensor(giants, device="cuda")).any())
            _same(edge_b - shift_t[owner], edge_a, "edge ids")
            far_ids += int((edge_b > (1 << 31)).sum())
        assert far_ids > 0


def test_weighted_hop_with_far_col_and_weights(oracle_mod, hiplib, far):
    """One weighted hop (fan-out 10): col is the first 2^31 + 2^16 int32 entries of the far buffer, the weights a float32
    allocation of its own of that size (8 GiB, NaN outside the real rows, freed right after); bands at entries 2^29, 2^30 and
    at the top, across 2^31.  Bit for bit the compact graph's picks; the compact run against the oracle as tests/
    test_gpu_weighted_golden.py compares long rows (libm may swap a near-tied pair)."""
    import torch
    from wholegraph_amd import wholegraph_ops as ops
    n = (1 << 31) + (1 << 16)
    col_far = fo.flat_view(far, torch.int32, n)
    rp, rp_far, col, bands, giants, shift = _far_csr(n, [1 << 29, 1 << 30], 3, max_deg=300)
    col = col.astype(np.int32)
    assert bands[-1][1] < (1 << 31) < bands[-1][1] + bands[-1][2]
    w = (np.random.default_rng(4).random(col.size) + 0.05).astype(np.float32)
    seeds = _sample_seeds(giants, 5, 400, np.int64)
    M, rs = 10, 4242
    cu = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    kw = dict(random_seed=rs, need_center_local_output=True, need_edge_output=True)
    want = [t.cpu().numpy() for t in ops.weighted_sample_without_replacement(cu(rp), cu(col), cu(w), cu(seeds), M, **kw)]
    ooff, odst, olid, ogid = oracle_mod.weighted_sample(rp, col, w, seeds, M, rs)
    assert np.array_equal(want[0], ooff) and np.array_equal(want[2], olid) and np.array_equal(col[want[3]], want[1])
    diff = sum(len(set(want[3][ooff[i]:ooff[i + 1]]) ^ set(ogid[ooff[i]:ooff[i + 1]])) for i in range(len(seeds)))
    assert diff <= 4, diff
    w_far = fo.far_buffer(n)
    try:
        wt = cu(w)
        for a, s, k in bands:
            w_far[s:s + k] = wt[a:a + k]
        with live_col(col_far, bands, col):
            got = [t.cpu().numpy() for t in ops.weighted_sample_without_replacement(cu(rp_far), col_far, w_far, cu(seeds), M, **kw)]
        _same_sample(got, want, seeds, shift, "weighted")
        assert got[3].max() > (1 << 31)
    finally:
        del w_far
        torch.cuda.empty_cache()


def test_the_far_buffer_is_left_as_it_was(far):
    """Every case clears the rows it placed: after the last one the whole buffer is NaN again (checked in 1 GiB pieces)."""
    import torch
    step = 1 << 28
    for lo in range(0, far.numel(), step):
        assert bool((far[lo:lo + step].view(torch.int32) == fo.NAN_BITS).all()), "live rows left behind near element %d" % lo
