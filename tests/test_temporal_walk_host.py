"""Host: the temporal hop of the call-group walk is exported, refuses a bad parameter block before anything touches a device
(``wgamd_sample_hop_pyg_temporal_nosync``), and ``NeighborSampler.temporal_call_groups_ok()`` says which temporal
configurations ``NeighborLoader.call_groups()`` takes while ``call_groups_ok()`` keeps its answer."""
import ctypes

import numpy as np
import pytest
import torch


def _block(L, at, M=10, max_row_len=100, edge_gid=True):
    from wholegraph_amd.fused import _PygHop
    # (host memory stands in for every array: the refusal comes before any pointer is followed)
    return _PygHop(at, at, L.DT_INT64, 1, M, at, at, at, at, 64, at, at, at, at, 64, at, at, at, at if edge_gid else None,
                   64 * M if M > 0 else 64, at, at, at, at, at, at, at, at, at, at, at, 1 << 20, None, 0, max_row_len, 1000, 0)


def test_temporal_hop_is_exported_and_refuses_bad_blocks_on_the_host(hiplib):
    from wholegraph_amd import _lib as L
    from wholegraph_amd.fused import TEMPORAL_COMPARISONS, _PygHopTime
    assert "wgamd_sample_hop_pyg_temporal_nosync" in L.SYMBOLS and "wgamd_sample_hop_temporal_workspace_bytes" in L.SYMBOLS
    assert TEMPORAL_COMPARISONS == {"strictly_increasing": 1, "monotonically_increasing": 2, "strictly_decreasing": 3,
                                    "monotonically_decreasing": 4}
    buf = np.zeros(4096, np.int64)
    at = buf.ctypes.data + (-buf.ctypes.data) % 256
    call = hiplib.wgamd_sample_hop_pyg_temporal_nosync
    ok_t = _PygHopTime(at, at, at, 4)
    ref = ctypes.byref
    bad = {
        "null parameter block": (None, ref(ok_t)),
        "null time block": (ref(_block(L, at)), None),
        "null csr_time": (ref(_block(L, at)), ref(_PygHopTime(None, at, at, 4))),
        "null frontier_time": (ref(_block(L, at)), ref(_PygHopTime(at, None, at, 4))),
        "null frontier_time_out": (ref(_block(L, at)), ref(_PygHopTime(at, at, None, 4))),
        "comparison 0": (ref(_block(L, at)), ref(_PygHopTime(at, at, at, 0))),
        "comparison 5": (ref(_block(L, at)), ref(_PygHopTime(at, at, at, 5))),
        "fan-out 257": (ref(_block(L, at, M=257)), ref(ok_t)),
        "fan-out 0": (ref(_block(L, at, M=0)), ref(ok_t)),
        "max_row_len 0": (ref(_block(L, at, max_row_len=0)), ref(ok_t)),
        "max_row_len -1": (ref(_block(L, at, max_row_len=-1)), ref(ok_t)),
        "null edge_gid": (ref(_block(L, at, edge_gid=False)), ref(ok_t)),
    }
    for what, (p, t) in bad.items():
        assert call(p, t, None) == L.WHOLEMEMORY_INVALID_INPUT, what
    # the workspace query: the biased hop's plan plus the picks before the time filter
    dt = L.DT_INT64
    plain = hiplib.wgamd_sample_hop_weighted_workspace_bytes(1000, 10000, dt, 500)
    need = hiplib.wgamd_sample_hop_temporal_workspace_bytes(1000, 10000, dt, 500)
    assert need >= plain + 10000 * 16 + 1001 * 4
    assert hiplib.wgamd_sample_hop_temporal_workspace_bytes(1000, 10000, dt, 0) == 0


def test_hop_workspace_sizes_are_pinned(hiplib):
    """The three workspace queries feed ``call_group_bytes_per_seed`` and ``HeteroNeighborSampler._walk_capacity_per_seed``
    and through them ``default_local_seeds_per_call``: the memory-sized call group of every loader that is given none, and
    the benchmark's ``--call-group`` default.  A change of these numbers changes what the loaders and the benchmark launch, so
    they are literals, taken from the library as it stood before this test; a change that means to move the default call group
    updates them knowingly."""
    from wholegraph_amd import _lib as L
    plain = hiplib.wgamd_sample_hop_workspace_bytes
    assert plain(4096, 102400, L.DT_INT64) == 6963968
    assert plain(4096, 102400, L.DT_INT) == 6554368
    assert plain(106496, 1024000, L.DT_INT64) == 70945280
    assert plain(106496, 1024000, L.DT_INT) == 66849280
    weighted, temporal = hiplib.wgamd_sample_hop_weighted_workspace_bytes, hiplib.wgamd_sample_hop_temporal_workspace_bytes
    assert weighted(106496, 1024000, L.DT_INT64, 500) == 75209472
    assert temporal(106496, 1024000, L.DT_INT64, 500) == 92019712
    assert weighted(106496, 1024000, L.DT_INT64, 20000) == 157125376
    assert temporal(106496, 1024000, L.DT_INT64, 20000) == 173935616


def _sampler(fanout, weights=None, **kw):
    from cugraph_pyg_amd.data.graph_store import CSRGraph
    from cugraph_pyg_amd.sampler.sampler import NeighborSampler
    row_ptr = torch.tensor([0, 2, 3, 3, 6])
    col = torch.tensor([1, 2, 0, 0, 1, 2])
    g = CSRGraph(row_ptr, col, torch.arange(6), None, weights, 4, torch.tensor([5, 1, 3, 3, 0, 9]))
    return NeighborSampler(g, fanout, biased=weights is not None, **kw)


def test_temporal_call_groups_ok_truth_table():
    pos, zero = torch.tensor([1., 2., 0.5, 1., 1., 3.]), torch.tensor([1., 0., 0.5, 1., 1., 3.])
    assert _sampler([3, 2], temporal=True).temporal_call_groups_ok()
    assert _sampler([1, 256], temporal=True).temporal_call_groups_ok()
    assert _sampler([3, 2], pos, temporal=True).temporal_call_groups_ok()
    assert _sampler([3, 2], pos.double(), temporal=True).temporal_call_groups_ok()
    assert not _sampler([3, 2], zero, temporal=True).temporal_call_groups_ok()          # zero weights
    assert not _sampler([3, 2], temporal=True, disjoint=True).temporal_call_groups_ok()
    assert not _sampler([3, 0], temporal=True).temporal_call_groups_ok()
    assert not _sampler([-1, 2], temporal=True).temporal_call_groups_ok()
    assert not _sampler([3, 257], temporal=True).temporal_call_groups_ok()
    assert not _sampler([3, 2]).temporal_call_groups_ok()                               # not temporal: the plain predicate's
    assert not _sampler([3, 2], pos).temporal_call_groups_ok()
    with pytest.raises(NotImplementedError):                                            # replacement is uniform, non-temporal
        _sampler([3, 2], temporal=True, with_replacement=True)
    s = _sampler([3, 2], temporal=True)
    s.with_replacement = True
    assert not s.temporal_call_groups_ok()


def test_call_groups_ok_stays_false_for_temporal_samplers():
    pos = torch.tensor([1., 2., 0.5, 1., 1., 3.])
    for kw in (dict(), dict(weights=pos), dict(disjoint=True)):
        assert not _sampler([3, 2], temporal=True, **kw).call_groups_ok()
    assert _sampler([3, 2]).call_groups_ok() and _sampler([3, 2], pos).call_groups_ok()
    # the routes that read it keep the one-batch-at-a-time plan for a temporal sampler
    s = _sampler([3, 2], temporal=True, local_seeds_per_call=64)
    assert s.fetch_plan(100, 16) == (0, 7, 7)
