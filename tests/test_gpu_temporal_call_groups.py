"""GPU: temporal neighbour sampling in call groups (``wgamd_sample_hop_pyg_temporal_nosync``, ``PygNoSyncWalk(csr_time=...)``,
``NeighborLoader(time_attr=..., input_time=...).call_groups()``).

The per-batch route is the definition: mini-batch b of a group must be, bit for bit, what
``sampler.neighbor_sample(graph, seeds_b, fanout, random_state + b, biased, False, seed_time_b, comparison)`` returns.

1. the walk against ``neighbor_sample`` on a graph with one vertex per degree at every boundary of the weighted sampler's
   size classes, seed times that put the number of qualifying slots at 0, 1, M - 1, M, M + 1 and N;
2. the loader: ``list(loader)`` against ``loader.call_groups()``, lazy against dense ``x`` through SAGE layers, and the seeds'
   outputs against the float64 per-batch formulation;
3. a check in numpy that trusts neither route: reach times replayed from the edge list, every sampled edge passes the
   comparison, every expanded centre has exactly min(q, fan-out) distinct slots, no centre is expanded twice;
4. what stays refused."""
import numpy as np
import pytest

from graphgen import powerlaw_csr

pytestmark = pytest.mark.gpu

FANOUTS = ([3, 2], [10, 5])
# every list class of the biased hop (wg_common.hpp: 16 / 32 / 64 / 128 / 256 / 512 / 1024 candidates), the one-wave cap
# (kWaveRowCap = 1024), the LDS key array (kWeightedLdsKeys = 12288) and the huge-row list (16384), plus M - 1, M, M + 1 for
# every fan-out in FANOUTS
DEGREES = sorted({0, 1, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 12288, 12289, 16384, 16385} |
                 {m + d for f in FANOUTS for m in f for d in (-1, 0, 1)})
COMPARISONS = ("monotonically_decreasing", "strictly_decreasing", "monotonically_increasing", "strictly_increasing")
_CMP = {"strictly_increasing": np.greater, "monotonically_increasing": np.greater_equal, "strictly_decreasing": np.less,
        "monotonically_decreasing": np.less_equal}
N_BATCHES = 8


def _branch_graph(comparison, weights):
    """One vertex per degree in DEGREES, columns drawn from the same vertex set.  ``monotonically_decreasing``: the time
    of a slot is its index in its row, so a seed time of q - 1 leaves exactly q qualifying slots; the other comparisons
    run on uniform random times in [0, 50) (ties abound)."""
    import torch
    from cugraph_pyg_amd.data.graph_store import CSRGraph
    rng = np.random.default_rng(11)
    V = len(DEGREES)
    deg = np.array(DEGREES, dtype=np.int64)
    row_ptr = np.zeros(V + 1, np.int64)
    row_ptr[1:] = np.cumsum(deg)
    E = int(row_ptr[-1])
    col = rng.integers(0, V, E).astype(np.int64)
    slot = np.arange(E) - np.repeat(row_ptr[:-1], deg)
    time = slot if comparison == "monotonically_decreasing" else rng.integers(0, 50, E)
    w = None
    if weights is not None:
        w64 = rng.random(E) * 3.0 + 0.05
        w = torch.from_numpy(w64.astype(np.float32) if weights == "float32" else w64).cuda()
    g = CSRGraph(torch.from_numpy(row_ptr).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(rng.permutation(E)).cuda(),
                 None, w, V, torch.from_numpy(time.astype(np.int64)).cuda())
    return g, deg


def _branch_seeds(comparison, deg, M):
    """N_BATCHES batches, every vertex once per batch.  ``monotonically_decreasing``: batch j puts q at the j-th of
    {0, 1, M - 1, M, M + 1, N} for every row (clipped to the row), the last two batches at random times."""
    rng = np.random.default_rng(5)
    V = deg.shape[0]
    seeds, times = [], []
    for j in range(N_BATCHES):
        perm = rng.permutation(V)
        if comparison == "monotonically_decreasing" and j < 6:
            q = np.minimum([0, 1, M - 1, M, M + 1, 1 << 40][j], deg[perm])
            t = q - 1
        else:
            t = rng.integers(0, 50, V)
        seeds.append(perm.astype(np.int64)), times.append(t.astype(np.int64))
    return seeds, times


_REFERENCE = {}


def _reference(comparison, fan_idx, weights):
    """(graph, seeds, times, per-batch neighbor_sample outputs), computed once per configuration and left unchanged."""
    import torch
    from cugraph_pyg_amd.sampler.sampler import neighbor_sample
    key = (comparison, fan_idx, weights)
    if key not in _REFERENCE:
        fanout = FANOUTS[fan_idx]
        g, deg = _branch_graph(comparison, weights)
        seeds, times = _branch_seeds(comparison, deg, fanout[0])
        outs = [neighbor_sample(g, torch.from_numpy(s).cuda(), fanout, 1000 + b, weights is not None, False,
                                torch.from_numpy(t).cuda(), comparison) for b, (s, t) in enumerate(zip(seeds, times))]
        _REFERENCE[key] = (g, seeds, times, outs)
    return _REFERENCE[key]


def _assert_batch_equal(got, want, what):
    import torch
    for k, name in enumerate(("node", "row", "col", "edge")):
        assert torch.equal(got[k].long(), want[k].long()), (what, name)
    assert [int(v) for v in got[4]] == [int(v) for v in want[4]], (what, "num_sampled_nodes")
    assert [int(v) for v in got[5]] == [int(v) for v in want[5]], (what, "num_sampled_edges")


def _run_walk(g, fanout, weights, comparison, G, compact_col, seeds, times, first_batch, lengths=None):
    """Batches first_batch .. first_batch + G of the configuration through one PygNoSyncWalk.run; ``lengths``: ragged lists."""
    import torch
    from cugraph_pyg_amd.sampler.sampler import hop_seed
    from wholegraph_amd.fused import PygNoSyncWalk
    B = seeds[0].shape[0]
    walk = PygNoSyncWalk(g.row_ptr, g.col, B, fanout, G, csr_weight=g.weight if weights is not None else None, pad_unique=False,
                         compact_col=compact_col, csr_time=g.time, temporal_comparison=comparison)
    rs = [[hop_seed(1000 + first_batch + j, k) for j in range(G)] for k in range(len(fanout))]
    if lengths is None:
        ids = torch.from_numpy(np.concatenate(seeds[first_batch:first_batch + G])).cuda()
        tms = torch.from_numpy(np.concatenate(times[first_batch:first_batch + G])).cuda()
        res = walk.run(ids, rs, seed_time=tms)
    else:
        ids, tms = np.zeros(G * B, np.int64), np.zeros(G * B, np.int64)
        seg = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
        batch = np.zeros(G * B, np.int32)
        for j, n in enumerate(lengths):
            ids[seg[j]:seg[j] + n], tms[seg[j]:seg[j] + n] = seeds[first_batch + j][:n], times[first_batch + j][:n]
            batch[seg[j]:seg[j] + n] = j
        res = walk.run(torch.from_numpy(ids).cuda(), rs, torch.from_numpy(seg).cuda(), torch.from_numpy(batch).cuda(),
                       seed_time=torch.from_numpy(tms).cuda())
    return res.finalize_batches(g.edge_id)


@pytest.mark.parametrize("weights", [None, "float32", "float64"])
@pytest.mark.parametrize("fan_idx", [0, 1])
@pytest.mark.parametrize("comparison", COMPARISONS)
def test_temporal_walk_equals_neighbor_sample_bit_for_bit(hiplib, comparison, fan_idx, weights):
    fanout = FANOUTS[fan_idx]
    g, seeds, times, want = _reference(comparison, fan_idx, weights)
    assert sum(int(o[5][0]) for o in want) > 0
    for G in (1, 4):
        for compact_col in (True, False):
            for b0 in range(0, N_BATCHES, G):
                got = _run_walk(g, fanout, weights, comparison, G, compact_col, seeds, times, b0)
                for j in range(G):
                    _assert_batch_equal(got[j], want[b0 + j], (G, compact_col, b0 + j))


@pytest.mark.parametrize("weights", [None, "float32"])
def test_temporal_walk_over_ragged_seed_lists(hiplib, weights):
    import torch
    from cugraph_pyg_amd.sampler.sampler import neighbor_sample
    comparison, fanout = "monotonically_decreasing", FANOUTS[1]
    g, seeds, times, _ = _reference(comparison, 1, weights)
    B = seeds[0].shape[0]
    lengths = [B, B - 7, 5, 1]
    got = _run_walk(g, fanout, weights, comparison, 4, True, seeds, times, 2, lengths)
    for j, n in enumerate(lengths):
        want = neighbor_sample(g, torch.from_numpy(seeds[2 + j][:n]).cuda(), fanout, 1000 + 2 + j, weights is not None, False,
                               torch.from_numpy(times[2 + j][:n]).cuda(), comparison)
        _assert_batch_equal(got[j], want, ("ragged", j))


def test_temporal_walk_batch_without_qualifying_edges(hiplib):
    """Batch 0 of the monotonically-decreasing configuration has q = 0 for every seed: no edges, later hops empty — inside
    a group whose other batches do sample."""
    g, seeds, times, want = _reference("monotonically_decreasing", 1, None)
    got = _run_walk(g, FANOUTS[1], None, "monotonically_decreasing", 4, True, seeds, times, 0)
    B = seeds[0].shape[0]
    assert [int(v) for v in got[0][4]] == [B, 0, 0] and [int(v) for v in got[0][5]] == [0, 0]
    assert got[0][1].numel() == 0 and got[0][0].cpu().tolist() == seeds[0].tolist()
    assert int(got[1][5][0]) > 0
    _assert_batch_equal(got[0], want[0], "q = 0")


# ---- 2. loader level ----------------------------------------------------------------------------------------------------------

def _temporal_loader_stores(V, F):
    import torch
    from cugraph_pyg_amd.data import FeatureStore, GraphStore
    row_ptr, col = powerlaw_csr(V, 14, seed=3, max_deg=600)
    dst = np.repeat(np.arange(V), np.diff(row_ptr))
    rng = np.random.default_rng(9)
    E = col.shape[0]
    gs, fs = GraphStore(), FeatureStore()
    gs[("n", "e", "n"), "coo", False, (V, V)] = torch.stack([torch.from_numpy(col.astype(np.int64)), torch.from_numpy(dst)]).cuda()
    feat = torch.from_numpy(rng.standard_normal((V, F)).astype(np.float32))
    fs["n", "x", None] = feat.cuda()
    fs["n", "y", None] = torch.arange(V, dtype=torch.int64).cuda()
    fs[("n", "e", "n"), "time", None] = torch.from_numpy(rng.integers(0, 100, E)).cuda()
    fs[("n", "e", "n"), "w", None] = torch.from_numpy((rng.random(E) + 0.05).astype(np.float32)).cuda()
    return gs, fs, feat


@pytest.mark.parametrize("fanout,dims", [([25, 10], [100, 256, 47]), ([7], [32, 64])])
@pytest.mark.parametrize("biased", [True, False])
@pytest.mark.parametrize("per_call", [4, 1])
def test_temporal_call_groups_equal_the_per_batch_loader_and_the_dense_formulation(hiplib, fanout, dims, biased, per_call):
    import torch
    from cugraph_pyg_amd.loader import NeighborLoader
    from test_gpu_call_group_loader import _forward, _model, _reference_seed_outputs
    V, B = 6000, 96
    gs, fs, feat = _temporal_loader_stores(V, dims[0])
    rng = np.random.default_rng(1)
    seeds = torch.from_numpy(rng.permutation(V)[:B * 9 + 17])                         # 9 full batches + a short one
    input_time = torch.from_numpy(rng.integers(0, 100, seeds.shape[0]))
    make = lambda: NeighborLoader((fs, gs), fanout, input_nodes=seeds, input_time=input_time, time_attr="time",  # noqa: E731
                                  weight_attr="w" if biased else None, batch_size=B, local_seeds_per_call=B * per_call,
                                  random_state=77)
    per_batch = list(make())
    groups = list(make().call_groups())
    assert sum(g.n_batches for g in groups) == len(per_batch) == 10
    assert [g.n_batches for g in groups] == [per_call] * (9 // per_call) + ([9 % per_call] if 9 % per_call else []) + [1]
    assert sum(int(d.edge_index.shape[1]) for d in per_batch) > 0
    convs = _model(dims, "cuda")
    at = 0
    for g in groups:
        datas = g.to_data_list()
        node_ptr, batch_ptr = g.node_ptr.tolist(), g.batch_ptr.tolist()
        for j, d in enumerate(datas):
            ref = per_batch[at + j]
            assert torch.equal(d.n_id, ref.n_id) and torch.equal(d.edge_index, ref.edge_index) and torch.equal(d.e_id, ref.e_id)
            assert torch.equal(d.x, ref.x) and torch.equal(d.y, ref.y) and torch.equal(d.input_id, ref.input_id)
            assert d.num_sampled_nodes.tolist() == ref.num_sampled_nodes.tolist()
            assert d.num_sampled_edges.tolist() == ref.num_sampled_edges.tolist()
            assert torch.equal(g.n_id[node_ptr[j]:node_ptr[j + 1]], ref.n_id)
        x_lazy, x_dense = g.x, g.node_attr("x", lazy=False)
        assert torch.equal(x_dense, feat[g.n_id.cpu()].cuda())
        out_lazy, out_dense = _forward(convs, g, x_lazy), _forward(convs, g, x_dense)
        assert out_lazy.shape == (g.num_seeds, dims[-1]) and torch.equal(out_lazy, out_dense)
        for j, d in enumerate(datas):
            want = _reference_seed_outputs(convs, d)
            got = out_lazy[batch_ptr[j]:batch_ptr[j + 1]].double().cpu()
            scale = float(want.abs().max()) + 1e-30
            assert float((got - want).abs().max()) <= 1e-5 * scale, (j, float((got - want).abs().max()), scale)
        at += g.n_batches
    assert at == len(per_batch)


# ---- 3. a check that trusts neither route ------------------------------------------------------------------------------------

@pytest.mark.parametrize("comparison,biased", [("monotonically_decreasing", False), ("strictly_increasing", True),
                                                ("strictly_decreasing", False), ("monotonically_increasing", True)])
def test_temporal_walk_replayed_on_the_host(hiplib, comparison, biased):
    import torch
    from cugraph_pyg_amd.sampler.sampler import hop_seed
    from wholegraph_amd.fused import PygNoSyncWalk
    V, B, G, fanout = 3000, 64, 4, [6, 4]
    row_ptr, col = powerlaw_csr(V, 12, seed=4, max_deg=400)
    rng = np.random.default_rng(2)
    E = col.shape[0]
    time = rng.integers(0, 60, E).astype(np.int64)
    w = (rng.random(E) + 0.05).astype(np.float32)
    seeds = rng.permutation(V)[:G * B].astype(np.int64)
    seed_time = rng.integers(0, 60, G * B).astype(np.int64)
    walk = PygNoSyncWalk(torch.from_numpy(row_ptr).cuda(), torch.from_numpy(col.astype(np.int64)).cuda(), B, fanout, G,
                         csr_weight=torch.from_numpy(w).cuda() if biased else None, pad_unique=False,
                         csr_time=torch.from_numpy(time).cuda(), temporal_comparison=comparison)
    rs = [[hop_seed(300 + j, k) for j in range(G)] for k in range(len(fanout))]
    outs = walk.run(torch.from_numpy(seeds).cuda(), rs, seed_time=torch.from_numpy(seed_time).cuda()).finalize_batches(None)
    cmp = _CMP[comparison]
    n_edges = 0
    for b, (node, row, colv, gid, nn, ne) in enumerate(outs):
        node, row, colv, gid = (t.cpu().numpy() for t in (node, row, colv, gid))
        assert node[:B].tolist() == seeds[b * B:(b + 1) * B].tolist() and len(set(node.tolist())) == node.shape[0]
        reach = {i: int(seed_time[b * B + i]) for i in range(B)}
        expanded = set()
        e0, f0, f1 = 0, 0, B
        for k, fan in enumerate(fanout):
            e1 = e0 + int(ne[k])
            slots_of = {}
            for e in range(e0, e1):
                c, r, s = int(colv[e]), int(row[e]), int(gid[e])
                assert f0 <= c < f1, "an edge's centre is a vertex of this hop's frontier"
                assert row_ptr[node[c]] <= s < row_ptr[node[c] + 1] and col[s] == node[r]
                assert cmp(time[s], reach[c]), "a sampled edge passes the comparison against its centre's reach time"
                slots_of.setdefault(c, []).append(s)
                if r not in reach:
                    reach[r] = int(time[s])      # the lowest-position incoming edge decides
            for c in range(f0, f1):           # every frontier vertex: exactly min(q, fan) distinct slots, q on the full graph
                lo, hi = row_ptr[node[c]], row_ptr[node[c] + 1]
                q = int(np.count_nonzero(cmp(time[lo:hi], reach[c])))
                got = slots_of.get(c, [])
                assert len(got) == len(set(got)) == min(q, fan), (b, k, c, q, len(got))
                assert got == sorted(got), "survivors stay in CSR order"
                assert c not in expanded
                expanded.add(c)
            e0, f0, f1 = e1, f1, f1 + int(nn[k + 1])
        assert e0 == row.shape[0] and f1 == node.shape[0] == len(reach)
        n_edges += e0
    assert n_edges > 0


# ---- 4. what stays refused ---------------------------------------------------------------------------------------------------

def test_temporal_call_groups_refusals(hiplib):
    import torch
    from cugraph_pyg_amd.data import FeatureStore, GraphStore
    from cugraph_pyg_amd.loader import NeighborLoader
    from cugraph_pyg_amd.loader.call_group import CallGroupIterator
    from cugraph_pyg_amd.loader.node_loader import NodeSamplerInput
    from cugraph_pyg_amd.sampler.sampler import NeighborSampler
    gs, fs, _ = _temporal_loader_stores(500, 8)
    seeds, t = torch.arange(64), torch.full((64,), 50)
    # input_time without time_attr
    with pytest.raises(NotImplementedError):
        NeighborLoader((fs, gs), [3, 3], input_nodes=seeds, input_time=t, batch_size=16).call_groups()
    # disjoint
    with pytest.raises(NotImplementedError):
        NeighborLoader((fs, gs), [3, 3], input_nodes=seeds, input_time=t, time_attr="time", batch_size=16, disjoint=True).call_groups()
    # fan-outs the temporal hop does not take
    with pytest.raises(NotImplementedError):
        NeighborLoader((fs, gs), [-1, 3], input_nodes=seeds, input_time=t, time_attr="time", batch_size=16).call_groups()
    # heterogeneous temporal
    hgs, hfs = GraphStore(), FeatureStore()
    hgs[("paper", "cites", "paper"), "coo", False, (4, 4)] = [torch.tensor([2, 1, 0, 0]), torch.tensor([3, 2, 1, 2])]
    hfs[("paper", "cites", "paper"), "time", None] = torch.tensor([0, 1, 2, 0])
    hgs[("author", "writes", "paper"), "coo", False, (3, 4)] = [torch.tensor([0, 0, 1, 1, 2, 2, 2]), torch.tensor([3, 2, 2, 1, 3, 2, 0])]
    hfs[("author", "writes", "paper"), "time", None] = torch.tensor([0, 0, 1, 0, 2, 1, 1])
    with pytest.raises(NotImplementedError):
        NeighborLoader((hfs, hgs), num_neighbors={("paper", "cites", "paper"): [2, 2], ("author", "writes", "paper"): [2, 2]},
                       batch_size=1, input_nodes=("paper", torch.tensor([3])), input_time=torch.tensor([-1]),
                       time_attr="time").call_groups()
    # seeds on the host
    graph = NeighborLoader((fs, gs), [3, 3], input_nodes=seeds, input_time=t, time_attr="time", batch_size=16)
    groups = graph.call_groups()            # (the loader itself moves its seeds to the device: this one is fine)
    smp = groups._smp
    assert isinstance(smp, NeighborSampler) and smp.temporal_call_groups_ok() and not smp.call_groups_ok()
    with pytest.raises(NotImplementedError):
        CallGroupIterator((fs, gs), smp, NodeSamplerInput(input_id=torch.arange(64), node=seeds, time=t, input_type=None), 1, 16)
