"""GPU: what the sampling kernels emit against the exact probability law of each sampler (``sampling_stats.py``) — the laws
``test_sampling_distribution_host.py`` holds the oracle to, asserted on the kernels' own output.

Slots are read from the returned CSR edge positions (edge_gid - row_ptr[row]).  Every vertex of a tier has the same degree,
so rows pool.  Every input is fixed; every bound is the 1e-6 quantile of the exact law.

1. the ABI ops, once per distinct kernel: uniform (register, workgroup and reservoir tiers), with replacement, weighted
   against the enumeration, one pick per size class, equal weights past the LDS key limit and in the huge-row list;
2. the call-group walk, plain and biased: G = 8 batches of B = 1024 seeds over a two-tier graph, per hop the marginal law, the
   pair law and independence between neighbouring local seeds, between neighbouring batches and between the hops;
3. the temporal walk (all four comparisons, plain and biased) and the per-batch temporal route: every returned edge passes the
   comparison against a reach time replayed in numpy, rows with q <= M return all q, rows with q > M follow the law."""
import numpy as np
import pytest

import sampling_stats as S
from sampling_stats import accept, replace_checks, size_class_weights, temporal_checks, uniform_checks

pytestmark = pytest.mark.gpu

N_ROWS = 8192
G, B = 8, 1024
W_1_TO_8 = np.arange(1, 9, dtype=np.float32)
W_NINE = np.array([0.05, 3, 0.5, 0.5, 1, 1, 2, 0.01, 0.2], dtype=np.float32)
_CMP = {"strictly_increasing": np.greater, "monotonically_increasing": np.greater_equal, "strictly_decreasing": np.less,
        "monotonically_decreasing": np.less_equal}


# ---- 1. the ABI ops -----------------------------------------------------------------------------------------------------------

def _op(kind, N, M, n, rs, seed_dtype, col_dtype, w=None):
    """One row of N slots sampled as n seeds of one call -> (offsets, local row of every pick, slot of every pick)."""
    import torch
    from wholegraph_amd import wholegraph_ops as ops
    rp = torch.tensor([0, N], dtype=torch.int64, device="cuda")
    col = torch.arange(N, dtype=col_dtype, device="cuda")
    seeds = torch.zeros(n, dtype=seed_dtype, device="cuda")
    if kind == "uniform":
        out = ops.unweighted_sample_without_replacement(rp, col, seeds, M, rs, True, True)
    elif kind == "replace":
        out = ops.unweighted_sample_with_replacement(rp, col, seeds, M, rs, True, True)
    else:
        weight = torch.from_numpy(np.ascontiguousarray(w)).cuda()
        out = ops.weighted_sample_without_replacement(rp, col, weight, seeds, M, rs, True, True)
    off, dst, lid, gid = (t.cpu().numpy() for t in out)
    assert np.array_equal(off, np.arange(n + 1) * M) and np.array_equal(dst, gid)       # col[j] = j
    return off, lid, gid


def _dtypes(i):
    import torch
    return [(torch.int64, torch.int64), (torch.int32, torch.int32), (torch.int64, torch.int32), (torch.int32, torch.int64)][i % 4]


@pytest.mark.parametrize("i,N,M,n", [(0, 40, 10, N_ROWS), (1, 33, 32, N_ROWS), (2, 200, 40, N_ROWS), (3, 600, 200, N_ROWS),
                                     (4, 3000, 1100, 2048)])
def test_abi_uniform_without_replacement(hiplib, i, N, M, n):
    off, lid, gid = _op("uniform", N, M, n, 777, *_dtypes(i))
    accept(uniform_checks(S.inclusion_matrix(lid, gid, n, N), M, N), f"gpu uniform ({N},{M}) n={n}")


@pytest.mark.parametrize("i,N,M", [(1, 7, 5), (2, 16, 10)])
def test_abi_uniform_with_replacement(hiplib, i, N, M):
    off, lid, gid = _op("replace", N, M, N_ROWS, 4242, *_dtypes(i))
    assert np.array_equal(lid, np.repeat(np.arange(N_ROWS), M)) and gid.min() >= 0 and gid.max() < N
    accept(replace_checks(gid.reshape(N_ROWS, M), N), f"gpu with replacement ({N},{M})")


@pytest.mark.parametrize("i,name,w,M", [(0, "1..8", W_1_TO_8, 3), (3, "nine", W_NINE, 4),
                                        (1, "nine f64", W_NINE.astype(np.float64), 4)])
def test_abi_weighted_against_enumeration(hiplib, i, name, w, M):
    n = 16384
    off, lid, gid = _op("weighted", len(w), M, n, 99, *_dtypes(i), w=w)
    a = S.inclusion_matrix(lid, gid, n, len(w))
    assert np.all(a.sum(1) == M)
    accept({"incl": S.incl_unequal(a.sum(0), n, S.weighted_inclusion(w, M))}, f"gpu weighted {name} M={M}")


@pytest.mark.parametrize("i,N", list(enumerate([17, 33, 65, 129, 257, 513, 1025])))
def test_abi_weighted_single_pick_per_size_class(hiplib, i, N):
    w = size_class_weights(N)
    off, lid, gid = _op("weighted", N, 1, N_ROWS, 99, *_dtypes(i), w=w)
    p = w.astype(np.float64) / w.astype(np.float64).sum()
    accept({"freq": S.multinomial(np.bincount(gid, minlength=N), N_ROWS * p, fold=True)}, f"gpu weighted M=1 N={N}")


@pytest.mark.parametrize("i,N", [(0, 12289), (1, 16385)])
def test_abi_weighted_equal_weights_on_long_rows(hiplib, i, N):
    """One past the LDS key array (12288) and one past the huge-row list (16384): 512 rows of 10 picks, 64 bins both ways."""
    n, M = 512, 10
    off, lid, gid = _op("weighted", N, M, n, 99, *_dtypes(i), w=np.full(N, 0.7, np.float32))
    a = S.inclusion_matrix(lid, gid, n, N)
    assert np.all(a.sum(1) == M)
    accept({"incl": S.incl(a.sum(0), n, M, N), "overlap(i,i+1)": S.overlap_shift(a, 1, M, N)},
           f"gpu weighted equal ({N},{M}) n={n}")


# ---- 2. the call-group walk ---------------------------------------------------------------------------------------------------

def _two_tier(N1, N2, seed=0):
    """G * B centres of degree N1 followed by B * N1 leaves of degree N2.  Centre c lists the N1 leaves of its class c mod B,
    so the centres of a batch (one per class) reach distinct leaves; leaf columns are random leaves."""
    C, n_leaf = G * B, B * N1
    deg = np.concatenate([np.full(C, N1), np.full(n_leaf, N2)]).astype(np.int64)
    row_ptr = np.zeros(C + n_leaf + 1, np.int64)
    row_ptr[1:] = np.cumsum(deg)
    e = np.arange(C * N1)
    col_c = C + ((e // N1) % B) * N1 + e % N1
    col_l = np.random.default_rng(seed).integers(C, C + n_leaf, n_leaf * N2)
    return row_ptr, np.concatenate([col_c, col_l]).astype(np.int64)


def _seeds():
    rng = np.random.default_rng(3)
    return np.concatenate([b * B + rng.permutation(B) for b in range(G)]).astype(np.int64)


def _batch(b):
    return slice(b * B, (b + 1) * B)


def _walk(row_ptr, col, fanout, rs0, id_dtype=np.int64, weight=None, time=None, comparison=None, seed_time=None, lengths=None):
    """The G batches through one PygNoSyncWalk.run -> finalize_batches(None) as numpy: [(node, row, col, gid, nn, ne)]."""
    import torch
    from cugraph_pyg_amd.sampler.sampler import hop_seed
    from wholegraph_amd.fused import PygNoSyncWalk
    dev = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda()      # noqa: E731
    walk = PygNoSyncWalk(dev(row_ptr), dev(col.astype(id_dtype)), B, fanout, G, csr_weight=dev(weight), pad_unique=False,
                         csr_time=dev(time), temporal_comparison=comparison)
    rs = [[hop_seed(rs0 + j, k) for j in range(G)] for k in range(len(fanout))]
    seeds = _seeds().astype(id_dtype)
    if lengths is None:
        res = walk.run(dev(seeds), rs, seed_time=dev(seed_time))
    else:
        seg = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
        ids, batch = np.zeros(G * B, id_dtype), np.zeros(G * B, np.int32)
        tms = None if seed_time is None else np.zeros(G * B, np.int64)
        for j, m in enumerate(lengths):
            ids[seg[j]:seg[j] + m], batch[seg[j]:seg[j] + m] = seeds[j * B:j * B + m], j
            if tms is not None:
                tms[seg[j]:seg[j] + m] = seed_time[j * B:j * B + m]
        res = walk.run(dev(ids), rs, dev(seg), dev(batch), seed_time=dev(tms))
    outs = res.finalize_batches(None)
    return [tuple(t.cpu().numpy() for t in o[:4]) + (list(o[4]), list(o[5])) for o in outs]


def _hops(outs, row_ptr, n_hops, time=None, seed_times=None):
    """Per hop, over all batches in order: the [rows, N] inclusion matrix of the frontier rows (a row that returned nothing is
    a zero row), the batch and the local index of every row and, for a temporal walk, the reach time of every row — replayed
    here: a seed's time, or the time of the first edge in the batch's list that reaches the vertex."""
    hops = [dict(a=[], batch=[], local=[], reach=[]) for _ in range(n_hops)]
    for b, (node, row, col, gid, nn, ne) in enumerate(outs):
        assert np.unique(node).shape[0] == node.shape[0] == sum(nn) and row.shape[0] == sum(ne)
        reach = None
        if time is not None:
            reach = np.full(node.shape[0], np.iinfo(np.int64).min)
            reach[:nn[0]] = seed_times[b]
        e0, f0, f1 = 0, 0, nn[0]
        for k in range(n_hops):
            e1 = e0 + ne[k]
            v = node[f0:f1]
            deg = row_ptr[v + 1] - row_ptr[v]
            N = int(deg[0]) if deg.shape[0] else 0
            assert np.all(deg == N), "one degree per tier"
            c = col[e0:e1] - f0
            assert np.all((0 <= c) & (c < f1 - f0)) and np.all(np.diff(c) >= 0), "a hop's edges follow its frontier"
            slot = gid[e0:e1] - row_ptr[v[c]]
            assert np.all((0 <= slot) & (slot < N))
            hops[k]["a"].append(S.inclusion_matrix(c, slot, f1 - f0, N))
            hops[k]["batch"].append(np.full(f1 - f0, b)), hops[k]["local"].append(np.arange(f1 - f0))
            if reach is not None:
                hops[k]["reach"].append(reach[f0:f1].copy())
                ids, first = np.unique(row[e0:e1], return_index=True)           # first edge that lists every neighbour
                new = ids >= f1
                assert np.array_equal(ids[new], np.arange(f1, f1 + nn[k + 1]))
                reach[ids[new]] = time[gid[e0:e1][first[new]]]
            e0, f0, f1 = e1, f1, f1 + nn[k + 1]
    return [{key: (np.concatenate(val) if val else None) for key, val in h.items()} for h in hops]


def _walk_hop_checks(h, M, N):
    """Marginal and pair law of one hop, independence between local seeds (i, i + 1) and (i, i + 64) of a batch and between
    batches b and b + 1 at equal local index."""
    a, batch = h["a"], h["batch"]
    n = a.shape[0]
    assert a.shape[1] == N and np.all(a.sum(1) == M)
    res = {"incl": S.incl(a.sum(0), n, M, N)}
    if M > 1:
        res["pair"] = S.pair(a, M, N)
    for s in (1, 64):
        i = np.nonzero(batch[:-s] == batch[s:])[0]
        res[f"overlap local(i,i+{s})"] = S.overlap(a[i], a[i + s], M, N)
    start = np.searchsorted(batch, np.arange(G + 1))
    m = np.minimum(np.diff(start)[:-1], np.diff(start)[1:])
    i = np.concatenate([start[b] + np.arange(m[b]) for b in range(G - 1)])
    j = np.concatenate([start[b + 1] + np.arange(m[b]) for b in range(G - 1)])
    res["overlap batch(b,b+1)"] = S.overlap(a[i], a[j], M, N)
    return res


WALKS = [  # fan-out, (N1, N2), id dtype, biased (equal weights), ragged
    ([10, 5], (40, 12), np.int64, False, False), ([15, 10], (40, 24), np.int32, False, False),
    ([25, 5], (40, 12), np.int64, False, False), ([8, 3], (40, 12), np.int32, False, False),
    ([10, 10], (40, 40), np.int64, False, False), ([10, 5], (40, 12), np.int64, False, True),
    ([10, 5], (40, 12), np.int32, True, False), ([10, 10], (40, 40), np.int64, True, False)]


@pytest.mark.parametrize("fanout,degrees,id_dtype,biased,ragged", WALKS)
def test_walk_hops_follow_the_uniform_law(hiplib, fanout, degrees, id_dtype, biased, ragged):
    row_ptr, col = _two_tier(*degrees)
    weight = np.full(col.shape[0], 0.7, np.float32) if biased else None
    lengths = [B, B - 7, B, 1000, B, B - 64, 999, B] if ragged else None
    outs = _walk(row_ptr, col, fanout, 777, id_dtype, weight=weight, lengths=lengths)
    hops = _hops(outs, row_ptr, 2)
    what = f"gpu walk {'biased ' if biased else ''}{'ragged ' if ragged else ''}{fanout} over {degrees}"
    n_seeds = sum(lengths) if ragged else G * B
    for k in range(2):
        assert hops[k]["a"].shape[0] == (n_seeds if k == 0 else n_seeds * fanout[0])
        accept(_walk_hop_checks(hops[k], fanout[k], degrees[k]), f"{what} hop {k + 1}")
    if fanout[0] == fanout[1] and degrees[0] == degrees[1]:      # hop 1 against hop 2 at equal local index
        first = hops[1]["local"] < B
        assert np.array_equal(hops[1]["batch"][first], hops[0]["batch"]) and np.array_equal(hops[1]["local"][first], hops[0]["local"])
        accept({"overlap hop(1,2)": S.overlap(hops[0]["a"], hops[1]["a"][first], fanout[0], degrees[0])}, f"{what} hops 1|2")


def test_biased_walk_single_pick_follows_the_weights(hiplib):
    """Fan-out [1] over centres of degree 65, every row with the same weights 0.05 + 3 u: slot j with probability w_j / sum w."""
    N = 65
    row_ptr, col = _two_tier(N, 0)
    w = size_class_weights(N)
    outs = _walk(row_ptr, col, [1], 777, weight=np.tile(w, G * B))
    h = _hops(outs, row_ptr, 1)[0]
    assert np.all(h["a"].sum(1) == 1)
    p = w.astype(np.float64) / w.astype(np.float64).sum()
    res = {"freq": S.multinomial(h["a"].sum(0), G * B * p, fold=True)}
    # rows 2k and 2k + 1 (one batch: B is even) are independent: the 4 x 4 table of their slots' quarters of the row
    quarter = (np.argmax(h["a"], axis=1) * 4) // N
    pq = np.bincount((np.arange(N) * 4) // N, weights=p, minlength=4)
    table = np.bincount(quarter[0::2] * 4 + quarter[1::2], minlength=16)
    res["quarters (2k,2k+1)"] = S.multinomial(table, np.outer(pq, pq).ravel() * (G * B // 2))
    accept(res, "gpu walk biased [1] N=65")


# ---- 3. temporal ----------------------------------------------------------------------------------------------------------------

def _seed_time(comparison, q, N):
    """The seed time that leaves exactly q qualifying slots in a row whose slot times are 0 .. N - 1."""
    return {"monotonically_decreasing": q - 1, "strictly_decreasing": q, "monotonically_increasing": N - q,
            "strictly_increasing": N - 1 - q}[comparison]


def _temporal_case(comparison, biased):
    """Centres and leaves of one degree N with slot time = slot index (the increasing comparisons qualify the last slots of a
    row, the decreasing ones the first); seed times that give q in {0, 1, M - 1, M, M + 1, 2M, N}, the last three four times
    as often, so that each pools 2048 rows."""
    N, M = (12, 3) if biased else (24, 5)
    row_ptr, col = _two_tier(N, N)
    time = (np.arange(col.shape[0]) % N).astype(np.int64)
    w = size_class_weights(N)
    weight = np.tile(w, col.shape[0] // N) if biased else None
    qs = np.array([0, 1, M - 1, M] + [M + 1] * 4 + [2 * M] * 4 + [N] * 4)
    q = qs[np.arange(G * B) % 16]
    seed_time = np.array([_seed_time(comparison, v, N) for v in range(N + 1)])[q].astype(np.int64)
    assert np.array_equal(_CMP[comparison](np.arange(N)[None, :], seed_time[:, None]).sum(1), q)
    return N, M, row_ptr, col, time, weight, (w if biased else None), seed_time


def _temporal_fanout(M):
    """The second hop draws fewer than the first, so that for the strict comparisons too some reach time with more
    qualifying slots than picks pools 2000 leaves (a leaf reached through slot s has s or s + 1 qualifying slots)."""
    return [M, M - 2 if M > 3 else M - 1]


def _temporal_assertions(hops, comparison, N, fanout, w, what):
    """Rows pool by reach time: same qualifying slots.  Every pool: nothing but qualifying slots, all q of them when q <= M,
    exactly M otherwise; pools of q > M with at least 2000 rows: the law."""
    for k, h in enumerate(hops):
        M = fanout[k]
        a, reach = h["a"], h["reach"]
        assert a.shape[1] == N and a.shape[0] >= N_ROWS
        lawful = set()
        for t in np.unique(reach):
            rows = reach == t
            ok = _CMP[comparison](np.arange(N), t)
            q, n = int(ok.sum()), int(rows.sum())
            law = q > M and n >= 2000
            res = temporal_checks(a[rows], ok, M, w, law=law)
            accept(res, f"{what} hop {k + 1} reach time {t}: q={q} rows={n}")
            if law:
                lawful.add(q)
        if k == 0:
            assert lawful == {M + 1, 2 * M, N}, lawful                      # the seeds' three pools of 2048
        else:
            assert lawful, "no pool of the second hop reached 2000 rows"


@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("comparison", sorted(_CMP))
def test_temporal_walk_follows_the_law_over_the_qualifying_slots(hiplib, comparison, biased):
    N, M, row_ptr, col, time, weight, w, seed_time = _temporal_case(comparison, biased)
    id_dtype = np.int32 if biased else np.int64
    fanout = _temporal_fanout(M)
    outs = _walk(row_ptr, col, fanout, 99, id_dtype, weight=weight, time=time, comparison=comparison, seed_time=seed_time)
    hops = _hops(outs, row_ptr, 2, time, [seed_time[_batch(b)] for b in range(G)])
    _temporal_assertions(hops, comparison, N, fanout, w, f"gpu temporal walk {'biased ' if biased else ''}{comparison}")


def test_per_batch_temporal_route_follows_the_law(hiplib):
    """``neighbor_sample(..., seed_time, comparison)``: the definition the walk is held to bit for bit gets the law too."""
    import torch
    from cugraph_pyg_amd.data.graph_store import CSRGraph
    from cugraph_pyg_amd.sampler.sampler import neighbor_sample
    comparison = "monotonically_decreasing"
    N, M, row_ptr, col, time, weight, w, seed_time = _temporal_case(comparison, False)
    g = CSRGraph(torch.from_numpy(row_ptr).cuda(), torch.from_numpy(col).cuda(), torch.arange(col.shape[0]).cuda(), None, None,
                 row_ptr.shape[0] - 1, torch.from_numpy(time).cuda())
    seeds, fanout = _seeds(), _temporal_fanout(M)
    outs = []
    for b in range(G):
        o = neighbor_sample(g, torch.from_numpy(seeds[_batch(b)]).cuda(), fanout, 99 + b, False, False,
                            torch.from_numpy(seed_time[_batch(b)]).cuda(), comparison)
        outs.append(tuple(t.cpu().numpy() for t in o[:4]) + (list(o[4]), list(o[5])))
    hops = _hops(outs, row_ptr, 2, time, [seed_time[_batch(b)] for b in range(G)])
    _temporal_assertions(hops, comparison, N, fanout, None, "gpu temporal per batch")
