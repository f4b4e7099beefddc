"""Host: the entries behind temporal heterogeneous / link call groups are exported and refuse null or inconsistent arguments
before anything touches a device (``wgamd_reach_time_append``, ``wgamd_rows_first_values``); ``graph_ops.rows_first_values`` off
the device is the torch formulation; ``HeteroNeighborSampler.temporal_call_groups_ok()`` says which temporal configurations the
link loaders' call groups take while ``call_groups_ok()`` keeps its answer; ``_walk_capacity_per_seed`` prices a temporal seed
higher and a non-temporal one as before."""
import numpy as np
import pytest
import torch

CITES, WRITES, REV = ("paper", "cites", "paper"), ("author", "writes", "paper"), ("paper", "rev_writes", "author")


def test_new_entries_refuse_bad_arguments_on_the_host(hiplib):
    from wholegraph_amd import _lib as L
    assert "wgamd_reach_time_append" in L.SYMBOLS and "wgamd_rows_first_values" in L.SYMBOLS
    buf = np.zeros(64, np.int64)     # (host memory stands in for every array: the refusal comes before any pointer is followed)
    at = buf.ctypes.data
    ok = dict(time_in=at, time_in_cap=8, node_seg=at, f_time=at, f_cap=8, f_seg=at, out_batch=at, out_seg=at, G=2, cap=16, out=at)
    order = ("time_in", "time_in_cap", "node_seg", "f_time", "f_cap", "f_seg", "out_batch", "out_seg", "G", "cap", "out")
    bad = [dict(time_in=None), dict(node_seg=None), dict(f_time=None), dict(f_seg=None), dict(out_batch=None), dict(out_seg=None),
           dict(out=None), dict(G=0), dict(G=1 << 20), dict(cap=0), dict(cap=1 << 30), dict(time_in_cap=-1), dict(f_cap=-1)]
    for change in bad:
        args = dict(ok, **change)
        assert hiplib.wgamd_reach_time_append(*(args[k] for k in order), None) == L.WHOLEMEMORY_INVALID_INPUT, change
    call = hiplib.wgamd_rows_first_values
    for what, args in {"null local": (None, at, at, 2, 4, at), "null seg": (at, None, at, 2, 4, at), "null values": (at, at, None, 2, 4, at),
                       "null out": (at, at, at, 2, 4, None), "no rows": (at, at, at, 0, 4, at), "empty rows": (at, at, at, 2, 0, at),
                       "rows past the domain": (at, at, at, 2, 8193, at), "too many elements": (at, at, at, 1 << 30, 4, at)}.items():
        assert call(*args, None) == L.WHOLEMEMORY_INVALID_INPUT, what


def test_rows_first_values_off_the_device_is_the_torch_formulation():
    from cugraph_pyg_amd.loader.link_loader import _batched_first_unique_torch, _first_occurrence
    from wholegraph_amd import graph_ops
    g = torch.Generator().manual_seed(3)
    for G, S, n_ids in ((1, 1, 4), (5, 65, 20), (3, 40, 1000), (2, 8193, 50)):      # (the last one: outside the kernel's domain)
        ends = torch.randint(0, n_ids, (G, S), generator=g)
        values = torch.randint(-(1 << 62), 1 << 62, (G, S), generator=g)
        uniq, seg, batch, local = _batched_first_unique_torch(ends, n_ids)
        got = graph_ops.rows_first_values(local, seg, values)
        assert got.dtype == torch.int64 and got.shape == (G * S,)
        seg_h = seg.tolist()
        for r in range(G):
            want = _first_occurrence(local[r], values[r], seg_h[r + 1] - seg_h[r])
            assert torch.equal(got[seg_h[r]:seg_h[r + 1]], want), (G, S, r)
        assert not bool(got[seg_h[G]:].any())


def _graph(n_dst, n_src, weights=None, time=True, col_dtype=torch.int64):
    from cugraph_pyg_amd.data.graph_store import CSRGraph
    deg = torch.arange(n_dst) % 4
    row_ptr = torch.zeros(n_dst + 1, dtype=torch.int64)
    row_ptr[1:] = torch.cumsum(deg, 0)
    E = int(row_ptr[-1])
    w = None if weights is None else (torch.ones(E) if weights == "positive" else torch.cat([torch.zeros(1), torch.ones(E - 1)]))
    return CSRGraph(row_ptr, (torch.arange(E) % n_src).to(col_dtype), torch.arange(E), None, w, n_dst,
                    (torch.arange(E) % 7) if time else None)


def _sampler(fan=None, weights=None, time=True, col_dtype=torch.int64, **kw):
    from cugraph_pyg_amd.sampler.sampler import HeteroNeighborSampler
    graphs = {CITES: _graph(12, 12, weights, time, col_dtype), WRITES: _graph(12, 5, weights, time, col_dtype),
              REV: _graph(5, 12, weights, time, col_dtype)}
    return HeteroNeighborSampler(graphs, fan or {CITES: [3, 2], WRITES: [2, 2], REV: [2, 1]}, biased=weights is not None, **kw)


def test_hetero_temporal_call_groups_ok_truth_table():
    assert _sampler(temporal=True).temporal_call_groups_ok()
    assert _sampler({CITES: [1, 256], WRITES: [2, 2], REV: [2, 0]}, temporal=True).temporal_call_groups_ok()     # a 0 skips a call
    assert _sampler(weights="positive", temporal=True).temporal_call_groups_ok()
    assert not _sampler(weights="zero", temporal=True).temporal_call_groups_ok()
    assert not _sampler(temporal=True, disjoint=True).temporal_call_groups_ok()
    assert not _sampler({CITES: [-1, 2], WRITES: [2, 2], REV: [2, 1]}, temporal=True).temporal_call_groups_ok()
    assert not _sampler({CITES: [3, 257], WRITES: [2, 2], REV: [2, 1]}, temporal=True).temporal_call_groups_ok()
    assert not _sampler(temporal=True, col_dtype=torch.int32).temporal_call_groups_ok()
    assert not _sampler().temporal_call_groups_ok() and not _sampler(weights="positive").temporal_call_groups_ok()   # not temporal
    with pytest.raises(NotImplementedError):                                            # replacement is uniform, non-temporal
        _sampler(temporal=True, with_replacement=True)
    with pytest.raises(ValueError):                                                     # an edge type without times
        _sampler(temporal=True, time=False)
    s = _sampler(temporal=True)
    s.with_replacement = True
    assert not s.temporal_call_groups_ok()
    # call_groups_ok() keeps its answer, and with it the routes that read it
    for kw in (dict(), dict(weights="positive"), dict(disjoint=True)):
        assert not _sampler(temporal=True, **kw).call_groups_ok()
    assert _sampler().call_groups_ok() and _sampler(weights="positive").call_groups_ok()
    assert _sampler(temporal=True, local_seeds_per_call=64).fetch_plan(100, 16) == (0, 7, 7)


def test_walk_capacity_per_seed_prices_the_time_lists(hiplib):
    from wholegraph_amd import _lib as L
    plain, temporal = _sampler(weights="positive"), _sampler(weights="positive", temporal=True)
    cost, cost_t = plain._walk_capacity_per_seed(), temporal._walk_capacity_per_seed()
    # a non-temporal sampler: the figure of the parent formula, recomputed here for the worst seed type
    fan, types, worst = plain.fanout, ["author", "paper"], None
    for seed_type in types:
        gained = {t: int(t == seed_type) for t in types}
        cap, total, ws, slots = dict(gained), 0.0, 0.0, 1
        for h in range(2):
            nxt = {t: 0 for t in types}
            for et in sorted(fan):
                fc = gained[et[2]]
                if fc == 0:
                    continue
                ec, nc = fc * fan[et][h], max(cap[et[0]], 1)
                total += ec * (4 * 4 + 8 + 8 + 4 + 8 + 4) + nc * (8 + 4) + (fc + 1) * 4
                ws = max(ws, hiplib.wgamd_sample_hop_workspace_bytes(4096 * max(nc, fc), 4096 * ec, L.DT_INT64) / 4096.0)
                slots = max(slots, nc + ec)
                cap[et[0]] += ec
                nxt[et[0]] += ec
            gained = nxt
        mine = (total + ws, slots, sum(cap.values()))
        worst = mine if worst is None or mine[0] > worst[0] else worst
    assert cost == worst
    # a temporal one: the same slots and rows, more bytes — at least 8 per node slot and per edge slot of capacity
    assert cost_t[1:] == cost[1:] and cost_t[0] > cost[0] + 8 * cost[2]
