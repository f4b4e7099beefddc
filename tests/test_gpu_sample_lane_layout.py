"""GPU parity of the one-seed-per-lane hop sampler (sample_uniform_lane_kernel, the no-sync walk's default for the fan-outs
5 / 10 / 15 / 25): every case is bit for bit the oracle's per-batch walk — target lists, per-hop CSR, renumber map, COO — at
the places where the lane layout can go wrong: degrees around the fan-out (every Fisher-Yates step finds its position or
its tail already touched), seed counts that do not fill a wave, batch boundaries inside a wave, live counts far below the
capacity, every id width, and stream numbers whose jump index has four non-zero bytes (the factored PCG jump).  Fan-outs
without a kernel of their own (7, 20) keep sample_uniform_multi_kernel and must give the same bits."""
import functools

import numpy as np
import pytest

from graphgen import powerlaw_csr, random_csr

pytestmark = pytest.mark.gpu

ID_WIDTHS = [(np.int64, True), (np.int64, False), (np.int32, True)]   # (id dtype, 32-bit column twin) as test_gpu_callgroup


def _oracle_batches(oracle_mod, row_ptr, col, seeds, G, B, fanouts, rs):
    return [oracle_mod.multilayer_sample(row_ptr, col, seeds[b * B:(b + 1) * B], fanouts, [rs[k][b] for k in range(len(fanouts))])
            for b in range(G)]


def _walk_equals(want, row_ptr, col, seeds, G, B, fanouts, rs, dtype=np.int64, compact=True):
    import torch
    from wholegraph_amd.fused import NoSyncWalk
    walk = NoSyncWalk(torch.from_numpy(row_ptr).cuda(), torch.from_numpy(col.astype(dtype)).cuda(), B, fanouts,
                      torch.from_numpy(seeds.astype(dtype)).dtype, G, compact_col=compact)
    per_batch = walk.run(torch.from_numpy(seeds.astype(dtype)).cuda(), rs).finalize_batches()
    assert len(per_batch) == G
    for b in range(G):
        for name, got_l, want_l in zip(("target_gids", "edge_indice", "csr_row_ptr", "csr_col_ind"), per_batch[b], want[b]):
            assert len(got_l) == len(want_l)
            for lvl, (x, y) in enumerate(zip(got_l, want_l)):
                assert np.array_equal(x.cpu().numpy(), y), (name, lvl, b)


# ---- degrees around the fan-out ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _degree_graph(M):
    """A few hundred rows of every degree M+1 .. 2M+1, some of 0, 1, M-1, M and 64, three of about 3000; rows shuffled."""
    rng = np.random.default_rng(1000 + M)
    deg = np.concatenate([np.repeat(np.arange(M + 1, 2 * M + 2), 200), np.repeat([0, 1, M - 1, M, 64], 24), [2990, 3000, 3011]])
    deg = rng.permutation(deg).astype(np.int64)
    row_ptr = np.zeros(deg.size + 1, np.int64)
    row_ptr[1:] = np.cumsum(deg)
    col = rng.integers(0, deg.size, row_ptr[-1]).astype(np.int64)
    G, B = 3, deg.size                                   # every row, in another order and under another seed per batch
    seeds = np.concatenate([rng.permutation(deg.size) for _ in range(G)]).astype(np.int64)
    rs = [[7919 * M + 31 * b + 5 for b in range(G)]]
    return row_ptr, col, seeds, G, B, rs


_degree_want = {}


@pytest.mark.parametrize("dtype,compact", ID_WIDTHS)
@pytest.mark.parametrize("M", [5, 10, 15, 25])
def test_degrees_around_the_fanout(oracle_mod, hiplib, M, dtype, compact):
    row_ptr, col, seeds, G, B, rs = _degree_graph(M)
    if M not in _degree_want:
        _degree_want[M] = _oracle_batches(oracle_mod, row_ptr, col, seeds, G, B, [M], rs)
    _walk_equals(_degree_want[M], row_ptr, col, seeds, G, B, [M], rs, dtype, compact)


# ---- odd sizes ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _powerlaw():
    return powerlaw_csr(20000, 18, seed=4, max_deg=3000)


@pytest.mark.parametrize("G,B", [(3, 1), (5, 37), (16, 64), (1, 1000)])
@pytest.mark.parametrize("fanouts", [[10, 5], [15, 10]])
def test_seed_counts_that_do_not_fill_a_wave(oracle_mod, hiplib, G, B, fanouts):
    row_ptr, col = _powerlaw()
    rng = np.random.default_rng(G * 1000 + B)
    seeds = np.concatenate([rng.permutation(20000)[:B] for _ in range(G)]).astype(np.int64)
    rs = [[900 * k + b + 11 for b in range(G)] for k in range(len(fanouts))]
    want = _oracle_batches(oracle_mod, row_ptr, col, seeds, G, B, fanouts, rs)
    _walk_equals(want, row_ptr, col, seeds, G, B, fanouts, rs)


def test_live_counts_far_below_the_capacity(oracle_mod, hiplib):
    """Degrees 0 .. 3 but for one row in fifty of degree 40: hop 2 holds about a tenth of the B x 15 entries its buffers are
    sized for, and most waves of both hops have no row longer than the fan-out and skip the draws."""
    rng = np.random.default_rng(8)
    V = 6000
    deg = rng.integers(0, 4, V)
    deg[rng.random(V) < 0.02] = 40
    row_ptr = np.zeros(V + 1, np.int64)
    row_ptr[1:] = np.cumsum(deg)
    col = rng.integers(0, V, row_ptr[-1]).astype(np.int64)
    G, B, fanouts = 4, 100, [15, 10]
    seeds = np.concatenate([rng.permutation(V)[:B] for _ in range(G)]).astype(np.int64)
    rs = [[70 * k + b + 1 for b in range(G)] for k in range(2)]
    want = _oracle_batches(oracle_mod, row_ptr, col, seeds, G, B, fanouts, rs)
    _walk_equals(want, row_ptr, col, seeds, G, B, fanouts, rs)


# ---- stream numbers past 2^24 -------------------------------------------------------------------------------------------------
def test_stream_numbers_past_2_to_24(oracle_mod, hiplib):
    """One batch of 530,000 seeds at fan-out 10: the seeds from 524,288 on draw from streams 32 i + t >= 2^24, and between
    them the stream numbers of the batch have every byte of the jump index non-zero."""
    V, B = 600000, 530000
    assert 32 * (B - 1) >= 1 << 24
    row_ptr, col = random_csr(V, 7000000, seed=33)      # average degree about 11: half the rows sample, half are copied
    seeds = np.random.default_rng(9).permutation(V)[:B].astype(np.int64)
    rs = [[12345678901]]
    want = _oracle_batches(oracle_mod, row_ptr, col, seeds, 1, B, [10], rs)
    _walk_equals(want, row_ptr, col, seeds, 1, B, [10], rs)


# ---- fan-outs that keep the lane-group kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fanouts", [[7], [20], [20, 7]])
def test_other_fanouts_keep_their_bits(oracle_mod, hiplib, fanouts):
    row_ptr, col = _powerlaw()
    G, B = 5, 37
    rng = np.random.default_rng(77)
    seeds = np.concatenate([rng.permutation(20000)[:B] for _ in range(G)]).astype(np.int64)
    rs = [[300 * k + b + 2 for b in range(G)] for k in range(len(fanouts))]
    want = _oracle_batches(oracle_mod, row_ptr, col, seeds, G, B, fanouts, rs)
    _walk_equals(want, row_ptr, col, seeds, G, B, fanouts, rs)
