"""GPU: a call group over a FeatureStore whose ``x`` is stored as float16 / bfloat16 (how the reference's examples store
features: ``--fp16_embedding``, ``--node_feat_format float16``, ``--dtype bfloat16``).  ``group.x`` is a ``LazyRows`` over the
16-bit table, and a two-layer ``nn.SAGEConv`` model over the group's layer graphs gives bit for bit the outputs of the same model
over a float32 store holding the same values: the first layer reads the 16-bit rows in its kernel and converts them exactly."""
import numpy as np
import pytest

from graphgen import powerlaw_csr

pytestmark = pytest.mark.gpu

V, F, FANOUT, BATCH, N_BATCHES = 2000, 100, [5, 3], 32, 4


def _stores(dtype):
    """(GraphStore, FeatureStore) with ``x`` = the same random values rounded to ``dtype``, stored as ``dtype`` or as float32."""
    import torch
    from cugraph_pyg_amd.data import FeatureStore, GraphStore
    row_ptr, col = powerlaw_csr(V, 10, seed=3, max_deg=300)
    dst = np.repeat(np.arange(V), np.diff(row_ptr))
    feat = torch.from_numpy(np.random.default_rng(3).standard_normal((V, F)).astype(np.float32)).to(dtype)
    out = []
    for stored in (dtype, torch.float32):
        gs, fs = GraphStore(), FeatureStore()
        gs[("n", "e", "n"), "coo", False, (V, V)] = torch.stack([torch.from_numpy(col.astype(np.int64)), torch.from_numpy(dst)]).cuda()
        fs["n", "x", None] = feat.to(stored).cuda()
        fs["n", "y", None] = torch.arange(V, dtype=torch.int64).cuda()
        out.append((gs, fs))
    return out


def _model(dims):
    import torch
    from wholegraph_amd import nn
    g = torch.Generator().manual_seed(5)
    convs = []
    for a, b in zip(dims[:-1], dims[1:]):
        c = nn.SAGEConv(a, b)
        for p in c.parameters():
            p.data = (torch.rand(p.shape, generator=g) - 0.5) * 0.4
        convs.append(c.cuda())
    return convs


@pytest.mark.parametrize("name", ["float16", "bfloat16"])
def test_call_group_over_a_16_bit_store(hiplib, name):
    import torch
    from cugraph_pyg_amd.loader import NeighborLoader
    from wholegraph_amd.nn import LazyRows
    dtype = getattr(torch, name)
    (gs16, fs16), (gs32, fs32) = _stores(dtype)
    seeds = torch.from_numpy(np.random.default_rng(1).permutation(V)[:BATCH * N_BATCHES])
    make = lambda fs, gs: NeighborLoader((fs, gs), FANOUT, input_nodes=seeds, batch_size=BATCH,  # noqa: E731
                                         local_seeds_per_call=BATCH * N_BATCHES, random_state=77)
    groups16, groups32 = list(make(fs16, gs16).call_groups()), list(make(fs32, gs32).call_groups())
    assert len(groups16) == len(groups32) == 1 and groups16[0].n_batches == N_BATCHES
    g16, g32 = groups16[0], groups32[0]
    assert torch.equal(g16.n_id, g32.n_id)
    x16, x32 = g16.x, g32.x
    assert isinstance(x16, LazyRows) and x16.table.dtype == dtype and x16.dtype == dtype
    assert isinstance(x32, LazyRows) and x32.table.dtype == torch.float32
    assert tuple(x16.shape) == (g16.num_nodes, F)
    convs = _model([F, 256, 47])
    with torch.no_grad():
        h16, h32 = x16, x32
        for j, c in enumerate(convs):
            act = "relu" if j + 1 < len(convs) else None
            h16, h32 = c(h16, g16.layer_graph(j), act=act), c(h32, g32.layer_graph(j), act=act)
            assert torch.equal(h16, h32), "layer %d" % j
    assert h16.shape == (g16.num_seeds, 47)
    assert x16._rows is None, "the first layer gathered the 16-bit rows instead of reading them in its kernel"
    rows = x16.materialize()
    assert rows.dtype == torch.float32 and torch.equal(rows, x32.materialize())
