"""GPU: the TEMPORAL heterogeneous call-group walk (``HeteroPygWalk(temporal_comparison=...)``: every (hop, edge type) call on
``wgamd_sample_hop_pyg_temporal_nosync``, a reach-time list per node type carried by ``wgamd_reach_time_append``).

The per-batch route is the definition: mini-batch j of a group must be, bit for bit, what ``sampler.hetero_neighbor_sample(graphs,
None, its seed lists, fanout, random_state + j, biased, its seed-time dict, comparison)`` returns — all six outputs.

1. the walk against ``hetero_neighbor_sample`` on a paper / author graph (``cites`` p->p, ``writes`` a->p, ``rev_writes`` p->a) with
   rows of degree 0, M - 1, M, M + 1 for every fan-out and one row of 1100 candidates (past the one-wave cap of the weighted
   sampler) in ``cites``, which is not the first edge type in sorted order; edge times in [0, 50), so ties abound; a fan-out of 0
   that skips a call; ragged seed lists of both node types and one type through ``seeds``; a batch that qualifies nothing;
2. that the configuration exercises what the time lists are for (asserted on the reference route's outputs): papers added through
   two edge types in one hop, vertices reached again after they are listed, rows with some but not all slots qualifying;
3. a replay in numpy that trusts neither route: reach times rebuilt from the edge lists per type, every sampled edge passes the
   comparison against its centre's reach time, every centre has exactly min(q, fan-out) distinct slots."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_P, N_A, B, N_BATCHES = 300, 100, 16, 4
CITES, WRITES, REV = ("paper", "cites", "paper"), ("author", "writes", "paper"), ("paper", "rev_writes", "author")
ETYPES = sorted([CITES, WRITES, REV])
FAN = {CITES: [3, 2], WRITES: [2, 2], REV: [2, 0]}
HUB, HUB_DEGREE = 7, 1100            # paper 7 has 1100 candidate slots in `cites`
COMPARISONS = ("monotonically_decreasing", "strictly_decreasing", "monotonically_increasing", "strictly_increasing")
_CMP = {"strictly_increasing": np.greater, "monotonically_increasing": np.greater_equal, "strictly_decreasing": np.less,
        "monotonically_decreasing": np.less_equal}
SEED0 = 1000
# ragged per-batch seed lists (papers, authors); the hub paper is the first paper of every list
LENGTHS = {"paper": [16, 9, 1, 12], "author": [5, 16, 7, 1]}
_GRAPHS, _REFERENCE = {}, {}


def _graphs(weights):
    """{edge type: CSRGraph} (rows = the destination type's vertices, columns = ids of the source type) and the same arrays
    in numpy; built once per weight kind and left unchanged."""
    if weights not in _GRAPHS:
        import torch
        from cugraph_pyg_amd.data.graph_store import CSRGraph
        rng = np.random.default_rng(23)
        graphs, host = {}, {}
        for et in ETYPES:
            n_src, n_dst = (N_P if et[0] == "paper" else N_A), (N_P if et[2] == "paper" else N_A)
            deg = rng.integers(0, 9, n_dst)
            deg[:6] = [0, 1, 2, 3, 4, 5]                   # 0 and M - 1, M, M + 1 for the fan-outs 2 and 3
            if et == CITES:
                deg[HUB] = HUB_DEGREE
            row_ptr = np.zeros(n_dst + 1, np.int64)
            row_ptr[1:] = np.cumsum(deg)
            E = int(row_ptr[-1])
            col = rng.integers(0, n_src, E).astype(np.int64)
            time = rng.integers(0, 50, E).astype(np.int64)
            edge_id = rng.permutation(E).astype(np.int64)
            w = (rng.random(E) * 3.0 + 0.05).astype(np.float32) if weights is not None else None
            graphs[et] = CSRGraph(torch.from_numpy(row_ptr).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(edge_id).cuda(),
                                  None, None if w is None else torch.from_numpy(w).cuda(), n_dst, torch.from_numpy(time).cuda())
            host[et] = dict(row_ptr=row_ptr, col=col, time=time, slot_of_edge=np.argsort(edge_id))
        assert ETYPES[0] != CITES
        _GRAPHS[weights] = (graphs, host)
    return _GRAPHS[weights]


def _seeds(comparison):
    """Per batch {type: (ids [B], times [B])}: B distinct vertices per type (ragged lists take a prefix).  Batch 0 starts at a
    time that qualifies no slot at all; the others at random times in [0, 50)."""
    rng = np.random.default_rng(5)
    nothing = -1 if "decreasing" in comparison else 50
    out = []
    for j in range(N_BATCHES):
        papers, authors = rng.permutation(N_P), rng.permutation(N_A)
        if j == 1:      # the rows of degree 0 .. 5 of every edge type (0 and M - 1, M, M + 1 for the fan-outs 2 and 3)
            papers = np.concatenate([np.arange(6), papers[papers >= 6]])
            authors = np.concatenate([np.arange(6), authors[authors >= 6]])
        papers = np.concatenate([[HUB], papers[papers != HUB][:B - 1]]).astype(np.int64)
        authors = authors[:B].astype(np.int64)
        times = {t: (np.full(B, nothing, np.int64) if j == 0 else rng.integers(0, 50, B).astype(np.int64)) for t in ("paper", "author")}
        out.append({"paper": (papers, times["paper"]), "author": (authors, times["author"])})
    return out


def _reference(comparison, weights):
    """(graphs, host arrays, seeds, per-batch reference outputs over the ragged lists of both types, per-batch reference outputs
    over the papers alone) — computed once per configuration and left unchanged."""
    key = (comparison, weights)
    if key not in _REFERENCE:
        import torch
        from cugraph_pyg_amd.sampler.sampler import hetero_neighbor_sample
        graphs, host = _graphs(weights)
        seeds = _seeds(comparison)
        both, papers = [], []
        for j, s in enumerate(seeds):
            ids = {t: torch.from_numpy(s[t][0][:LENGTHS[t][j]]).cuda() for t in s}
            tms = {t: torch.from_numpy(s[t][1][:LENGTHS[t][j]]).cuda() for t in s}
            both.append(hetero_neighbor_sample(graphs, None, ids, FAN, SEED0 + j, weights is not None, tms, comparison))
            papers.append(hetero_neighbor_sample(graphs, "paper", torch.from_numpy(s["paper"][0]).cuda(), FAN, SEED0 + j,
                                                 weights is not None, torch.from_numpy(s["paper"][1]).cuda(), comparison))
        _REFERENCE[key] = (graphs, host, seeds, both, papers)
    return _REFERENCE[key]


def _random_seeds(first_batch, G):
    import torch
    from cugraph_pyg_amd.sampler.sampler import _as_i64, hop_seed
    return torch.tensor([[_as_i64(hop_seed(SEED0 + first_batch + j, k)) for j in range(G)] for k in range(2 * len(ETYPES))],
                        dtype=torch.int64)


def _walk(graphs, weights, comparison, G):
    from wholegraph_amd.fused import HeteroPygWalk
    return HeteroPygWalk(graphs, B, FAN, G, biased=weights is not None, num_nodes={"paper": N_P, "author": N_A}, pad_unique=False,
                         temporal_comparison=comparison)


def _run_lists(graphs, weights, comparison, seeds, first_batch, G):
    """Batches first_batch .. first_batch + G over the ragged lists of both node types, times as the lists' fourth entry."""
    import torch
    lists = {}
    for t in ("paper", "author"):
        n = LENGTHS[t][first_batch:first_batch + G]
        seg = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
        ids, tms, batch = np.zeros(G * B, np.int64), np.zeros(G * B, np.int64), np.zeros(G * B, np.int32)
        for j in range(G):
            ids[seg[j]:seg[j + 1]] = seeds[first_batch + j][t][0][:n[j]]
            tms[seg[j]:seg[j + 1]] = seeds[first_batch + j][t][1][:n[j]]
            batch[seg[j]:seg[j + 1]] = j
        lists[t] = tuple(torch.from_numpy(a).cuda() for a in (ids, seg, batch, tms))
    walk = _walk(graphs, weights, comparison, G)
    rec = walk.run(None, None, _random_seeds(first_batch, G), seed_lists=lists)
    return walk.finalize_batches(rec), rec


def _assert_batch_equal(got, want, what):
    import torch
    for k, name in enumerate(("node", "row", "col", "edge")):
        assert sorted(got[k]) == sorted(want[k]), (what, name)
        for key in want[k]:
            assert torch.equal(got[k][key].long(), want[k][key].long()), (what, name, key)
    for k, name in ((4, "num_sampled_nodes"), (5, "num_sampled_edges")):
        assert sorted(got[k]) == sorted(want[k]), (what, name)
        for key in want[k]:
            assert [int(v) for v in got[k][key]] == [int(v) for v in want[k][key]], (what, name, key)


@pytest.mark.parametrize("weights", [None, "float32"])
@pytest.mark.parametrize("comparison", COMPARISONS)
def test_hetero_temporal_walk_equals_hetero_neighbor_sample_bit_for_bit(hiplib, comparison, weights):
    import torch
    graphs, host, seeds, both, papers = _reference(comparison, weights)
    assert sum(sum(o[5][et][0] for et in ETYPES) for o in both) > 0
    for G in (1, 4):
        for b0 in range(0, N_BATCHES, G):
            got, rec = _run_lists(graphs, weights, comparison, seeds, b0, G)
            for j in range(G):
                _assert_batch_equal(got[j], both[b0 + j], ("lists", G, b0 + j))
            # the reach-time lists run parallel to the vertex lists
            for t in ("paper", "author"):
                st = rec["state"][t]
                assert st["time"].dtype == torch.int64 and st["time"].shape[0] >= int(st["seg"][-1])
        # one seed type through `seeds` / `seed_time`
        for b0 in range(0, N_BATCHES, G):
            ids = torch.from_numpy(np.concatenate([seeds[b0 + j]["paper"][0] for j in range(G)])).cuda()
            tms = torch.from_numpy(np.concatenate([seeds[b0 + j]["paper"][1] for j in range(G)])).cuda()
            walk = _walk(graphs, weights, comparison, G)
            got = walk.finalize_batches(walk.run("paper", ids, _random_seeds(b0, G), seed_time=tms))
            for j in range(G):
                _assert_batch_equal(got[j], papers[b0 + j], ("seeds", G, b0 + j))


def test_hetero_temporal_walk_batch_without_qualifying_edges(hiplib):
    """Batch 0 starts at a time no slot qualifies against: no edges and no new vertices of any type, inside a group whose other
    batches do sample."""
    comparison = "monotonically_decreasing"
    graphs, host, seeds, both, _ = _reference(comparison, None)
    got, _ = _run_lists(graphs, None, comparison, seeds, 0, 4)
    node, row, col, edge, nn, ne = got[0]
    assert all(v.numel() == 0 for v in row.values()) and all(sum(v) == 0 for v in ne.values())
    assert [int(v) for v in nn["paper"]] == [LENGTHS["paper"][0], 0, 0] and [int(v) for v in nn["author"]] == [LENGTHS["author"][0], 0, 0]
    assert node["paper"].cpu().tolist() == seeds[0]["paper"][0][:LENGTHS["paper"][0]].tolist()
    assert sum(sum(v) for v in got[1][5].values()) > 0
    _assert_batch_equal(got[0], both[0], "q = 0")


def test_hetero_temporal_walk_needs_its_times(hiplib):
    import torch
    graphs, _ = _graphs(None)
    ids = torch.arange(B, dtype=torch.int64).cuda()
    with pytest.raises(ValueError, match="temporal"):
        _walk(graphs, None, "monotonically_decreasing", 1).run("paper", ids, _random_seeds(0, 1))
    with pytest.raises(ValueError, match="temporal"):
        _walk(graphs, None, None, 1).run("paper", ids, _random_seeds(0, 1), seed_time=ids)
    with pytest.raises(ValueError, match="temporal_comparison"):
        _walk(graphs, None, "sometimes", 1)


# ---- the replay ------------------------------------------------------------------------------------------------------------

def _replay(host, comparison, out, seed_times):
    """One mini-batch's six outputs replayed on the host from the edge lists alone.  Returns (expanded rows, rows with
    0 < q < N, edges that reach a vertex already listed, (papers added by cites, papers added by rev_writes) in the first hop)."""
    cmp = _CMP[comparison]
    node, row, col, edge, nn, ne = [{k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in o.items()} for o in out]
    reach = {t: [int(v) for v in seed_times[t]] for t in ("paper", "author")}
    for t in reach:
        assert int(nn[t][0]) == len(reach[t]) and len(set(node[t].tolist())) == node[t].shape[0]
    front = {t: (0, len(reach[t])) for t in reach}
    at = {et: 0 for et in ETYPES}
    expanded = partial = again = 0
    added_h0 = {}
    for h in range(2):
        begin = {t: len(reach[t]) for t in reach}
        for et in ETYPES:
            src_t, _, dst_t = et
            fan, n_e = FAN[et][h], int(ne[et][h])
            f0, f1 = front[dst_t]
            if fan == 0 or f1 == f0:
                assert n_e == 0
                continue
            g = host[et]
            slots_of, before = {}, len(reach[src_t])
            for e in range(at[et], at[et] + n_e):
                c, r, s = int(col[et][e]), int(row[et][e]), int(g["slot_of_edge"][int(edge[et][e])])
                assert f0 <= c < f1, "an edge's centre is a vertex of this hop's frontier of the destination type"
                v = int(node[dst_t][c])
                assert g["row_ptr"][v] <= s < g["row_ptr"][v + 1] and g["col"][s] == node[src_t][r]
                assert cmp(g["time"][s], reach[dst_t][c]), "a sampled edge passes the comparison against its centre's reach time"
                slots_of.setdefault(c, []).append(s)
                if r == len(reach[src_t]):
                    reach[src_t].append(int(g["time"][s]))      # first appearance: the lowest-position edge decides
                else:
                    assert r < len(reach[src_t]), "new vertices are numbered in first-appearance order"
                    again += r < before
            for c in range(f0, f1):
                v = int(node[dst_t][c])
                lo, hi = g["row_ptr"][v], g["row_ptr"][v + 1]
                q = int(np.count_nonzero(cmp(g["time"][lo:hi], reach[dst_t][c])))
                got = slots_of.get(c, [])
                assert len(got) == len(set(got)) == min(q, fan), (h, et, c, q, len(got))
                assert got == sorted(got), "survivors stay in CSR order"
                expanded += 1
                partial += 0 < q < hi - lo
            at[et] += n_e
            if h == 0:
                added_h0[et] = len(reach[src_t]) - before
        for t in reach:
            assert len(reach[t]) - begin[t] == int(nn[t][h + 1])
            front[t] = (begin[t], len(reach[t]))
    for t in reach:
        assert len(reach[t]) == node[t].shape[0]
    for et in ETYPES:
        assert at[et] == row[et].shape[0]
    return expanded, partial, again, (added_h0.get(CITES, 0), added_h0.get(REV, 0))


def _list_times(seeds, j):
    return {t: seeds[j][t][1][:LENGTHS[t][j]] for t in ("paper", "author")}


@pytest.mark.parametrize("comparison,weights", [("monotonically_decreasing", None), ("strictly_increasing", "float32"),
                                                ("strictly_decreasing", None), ("monotonically_increasing", "float32")])
def test_hetero_temporal_configuration_is_not_vacuous_and_replays_on_the_host(hiplib, comparison, weights):
    graphs, host, seeds, both, _ = _reference(comparison, weights)
    # the reference route's outputs: what the time lists are for does happen
    stats = [_replay(host, comparison, both[j], _list_times(seeds, j)) for j in range(N_BATCHES)]
    assert any(s[3][0] > 0 and s[3][1] > 0 for s in stats), "no batch adds papers through both cites and rev_writes in one hop"
    assert sum(s[2] for s in stats) > 0, "no vertex is reached again after it is listed"
    assert 4 * sum(s[1] for s in stats) >= sum(s[0] for s in stats) > 0, "fewer than a quarter of the rows have 0 < q < N"
    # the walk's outputs, replayed the same way
    got, _ = _run_lists(graphs, weights, comparison, seeds, 0, 4)
    assert sum(_replay(host, comparison, got[j], _list_times(seeds, j))[0] for j in range(N_BATCHES)) > 0
