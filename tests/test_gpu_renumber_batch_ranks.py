"""Per-batch first-appearance ranks of the call-group renumbering (WGAMD_HOP_UNIFORM_BATCHES): a hop whose batches are
promised uniform counts every batch's new vertices in the table kernel and resolves the ranks inside a batch in the emit
kernel's LDS — three launches per hop.  Every mini-batch must still be exactly the oracle's single-batch walk, the call
without the promise (today's path: bits and running counts over the whole edge array) must give the same tensors, and the
shapes below are the smallest at which the new code can go wrong: batches shorter than a 64-edge word, parts whose
boundaries are not word-aligned, three hops, split and multi-trip hash ranges, batches without edges or without new
vertices, repeats whose first position lies in an earlier part, a window just too large for LDS, replays.

Each test starts ONE fresh child process (the library reads its environment knobs once per process)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_WORKER = r"""
import sys
import numpy as np, torch
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, root + "/cugraph-gnn_amd"); sys.path.insert(0, root + "/tests")
import oracle
from graphgen import powerlaw_csr
from wholegraph_amd.fused import NoSyncWalk, PygNoSyncWalk, CapturedWalk, HOP_UNIFORM_BATCHES
oracle.build()
_graphs = {}


def graph(dtype, n=30000):
    if (dtype, n) not in _graphs:
        _graphs[(dtype, n)] = powerlaw_csr(n, 18, seed=11, col_dtype=dtype, max_deg=3000)
    return _graphs[(dtype, n)]


def check_oracle(row_ptr, col, seeds, G, B, fanouts, rs, per_batch):
    for b in range(G):
        want = oracle.multilayer_sample(row_ptr, col, seeds[b * B:(b + 1) * B], fanouts, [rs[k][b] for k in range(len(fanouts))])
        for name, got_l, want_l in zip(("target_gids", "edge_indice", "csr_row_ptr", "csr_col_ind"), per_batch[b], want):
            for lvl, (x, y) in enumerate(zip(got_l, want_l)):
                assert np.array_equal(x.cpu().numpy(), y), (name, lvl, b, G, B, fanouts)


def live(res):
    # everything a consumer of the walk can see below the live ends, per hop
    out = []
    for k in range(res.hops):
        n_e, n_u = res.counts[k].cpu().tolist()
        n_t = int(res.target_seg[k][-1])
        out.append((res.counts[k].clone(), res.unique_seg[k].clone(), res.unique[k][:n_u].clone(), res.unique[k][n_u:].clone(),
                    res.neighbor_row[k][:n_e].clone(), res.center_row[k][:n_e].clone(), res.offsets[k][:n_t + 1].clone(),
                    None if k + 1 == res.hops else res.target_batch[k + 1][:n_u].clone()))
    return out


def same(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        for i, (u, v) in enumerate(zip(x, y)):
            assert (u is None and v is None) or torch.equal(u, v), (k, i)


def run_walk(row_ptr, col, dtype, G, B, fanouts, compact, seeds=None, against_plain=True):
    rng = np.random.default_rng(G + B)
    if seeds is None:
        seeds = np.concatenate([rng.permutation(row_ptr.size - 1)[:B] for _ in range(G)]).astype(dtype)   # batches overlap
    rs = [[500 * k + b + 3 for b in range(G)] for k in range(len(fanouts))]
    rp_d, col_d, seeds_d = torch.from_numpy(row_ptr).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(seeds).cuda()
    walk = NoSyncWalk(rp_d, col_d, B, fanouts, seeds_d.dtype, G, compact_col=compact)
    assert walk.flags & HOP_UNIFORM_BATCHES
    res = walk.run(seeds_d, rs)
    check_oracle(row_ptr, col, seeds, G, B, fanouts, rs, res.finalize_batches())
    got = live(res)
    if against_plain:   # the same call without the promise: every tensor identical, the -1 padding included
        plain = NoSyncWalk(rp_d, col_d, B, fanouts, seeds_d.dtype, G, compact_col=compact)
        plain.flags &= ~HOP_UNIFORM_BATCHES
        same(got, live(plain.run(seeds_d, rs)))
    return walk, seeds_d, rs, got


def case_short_batches():       # 1: 35 / 210 edges per batch: word boundaries fall inside and across batches
    row_ptr, col = graph(np.int32)
    run_walk(row_ptr, col, np.int32, 9, 7, [5, 5], True)


def case_three_hops():          # 2: int64 ids, three hops, part boundaries that are not word-aligned
    row_ptr, col = graph(np.int64)
    run_walk(row_ptr, col, np.int64, 3, 200, [15, 10, 5], True)


def case_products_shape():      # 3 (and 4 under WGAMD_RENUMBER_KEYS_TARGET): int32 / int64, with and without the 32-bit columns
    for dtype, compact in ((np.int32, True), (np.int64, True), (np.int64, False)):
        row_ptr, col = graph(dtype)
        run_walk(row_ptr, col, dtype, 6, 256, [25, 10], compact)


def case_empty_and_hub():       # 5
    row_ptr, col = graph(np.int64)
    V, G, B, fanouts = row_ptr.size - 1, 5, 64, [10, 10]
    rng = np.random.default_rng(17)
    # a batch whose seeds all have degree 0 (their rows removed from the CSR): no edges, no new vertices, an empty stretch
    # between two live batches
    lonely = rng.permutation(V)[:B]
    deg = np.diff(row_ptr)
    keep = np.ones(col.size, bool)
    for v in lonely:
        keep[row_ptr[v]:row_ptr[v + 1]] = False
    deg2 = deg.copy()
    deg2[lonely] = 0
    rp2 = np.zeros(V + 1, np.int64)
    rp2[1:] = np.cumsum(deg2)
    col2 = col[keep]
    seeds = np.concatenate([rng.permutation(V)[:B] for _ in range(G)]).astype(np.int64)
    seeds[2 * B:3 * B] = lonely
    run_walk(rp2, col2, np.int64, G, B, fanouts, True, seeds=seeds)
    # a batch whose seeds are all neighbours of one hub: their neighbourhoods repeat each other, so most of the batch's
    # 7,040 hop-2 edges are repeats whose first position lies in an earlier part
    hub = int(np.argmax(deg))
    around = np.unique(col[row_ptr[hub]:row_ptr[hub + 1]])
    assert around.size >= B
    seeds = np.concatenate([rng.permutation(V)[:B] for _ in range(G)]).astype(np.int64)
    seeds[1 * B:2 * B] = around[:B]
    seeds[4 * B:5 * B] = around[-B:]
    run_walk(row_ptr, col, np.int64, G, B, fanouts, True, seeds=seeds)


def case_pyg():                 # 6
    from test_gpu_pyg_loader import oracle_neighbor_sample
    from cugraph_pyg_amd.sampler.sampler import hop_seed
    G, B, fanouts = 6, 100, [25, 10]
    row_ptr, col = powerlaw_csr(15000, 14, seed=8, col_dtype=np.int64, max_deg=2500)
    eid = np.random.default_rng(3).permutation(col.size).astype(np.int64)
    rng = np.random.default_rng(G + B)
    seeds = np.concatenate([rng.permutation(15000)[:B] for _ in range(G)]).astype(np.int64)
    rstate = [500 + b for b in range(G)]
    rs = [[hop_seed(rstate[b], k) for b in range(G)] for k in range(len(fanouts))]
    walk = PygNoSyncWalk(torch.from_numpy(row_ptr).cuda(), torch.from_numpy(col).cuda(), B, fanouts, G)

    def check(res, lists):
        per_batch = res.finalize_batches(torch.from_numpy(eid).cuda())
        for b in range(G):
            node, row, colv, edge, nn, ne = oracle_neighbor_sample(oracle, row_ptr, col, eid, lists[b], fanouts, rstate[b])
            g_node, g_row, g_col, g_edge, g_nn, g_ne = per_batch[b]
            assert np.array_equal(g_node.cpu().numpy(), node)
            assert np.array_equal(g_row.cpu().numpy(), row) and np.array_equal(g_col.cpu().numpy(), colv)
            assert np.array_equal(g_edge.cpu().numpy(), edge)
            assert g_nn == nn and g_ne == ne

    def pyg_live(res):
        out = [res.counts.clone(), res.node_seg.clone(), res.nodes[:int(res.node_seg[-1])].clone()]
        for k in range(res.hops):
            n_e = int(res.counts[k][0])
            out += [res.row_local[k][:n_e].clone(), res.col_local[k][:n_e].clone(), res.edge_gid[k][:n_e].clone(),
                    res.frontier_seg[k + 1].clone(), res.frontier_local0[k].clone()]
        return out

    # uniform batches: the promise is made, the ranks are resolved per batch
    uniform = walk.run(torch.from_numpy(seeds).cuda(), rs)
    check(uniform, [seeds[b * B:(b + 1) * B] for b in range(G)])
    # the same segments handed in by the caller: no promise, today's path, the same tensors
    explicit = walk.run(torch.from_numpy(seeds).cuda(), rs, seed_seg=walk.seed_seg.clone(), seed_batch=walk.seed_batch.clone())
    for i, (u, v) in enumerate(zip(pyg_live(uniform), pyg_live(explicit))):
        assert torch.equal(u, v), i
    # an uneven seed_seg: no promise either
    sizes = [B, B - 37, 3, B, 1, B - 8]
    lists = [seeds[b * B:b * B + sizes[b]] for b in range(G)]
    ragged = np.zeros(G * B, np.int64)
    seg = np.zeros(G + 1, np.int32)
    seg[1:] = np.cumsum(sizes)
    ragged[:seg[G]] = np.concatenate(lists)
    batch = np.zeros(G * B, np.int32)
    batch[:seg[G]] = np.repeat(np.arange(G, dtype=np.int32), sizes)
    uneven = walk.run(torch.from_numpy(ragged).cuda(), rs, seed_seg=torch.from_numpy(seg).cuda(), seed_batch=torch.from_numpy(batch).cuda())
    check(uneven, lists)


def case_window_too_large():    # 7: 128 x 52 x 53 = 352,768 hop-2 edges per batch: 5,513 words x 12 B = 66,156 B > 65,536 B of window
    row_ptr, col = graph(np.int64)
    run_walk(row_ptr, col, np.int64, 3, 128, [51, 53], True, against_plain=False)


def case_replay():              # 8: the counters are cleared by the launch chain itself
    row_ptr, col = graph(np.int64)
    walk, seeds_d, rs, first = run_walk(row_ptr, col, np.int64, 6, 256, [25, 10], True, against_plain=False)
    same(first, live(walk.run(seeds_d, rs)))
    cap = CapturedWalk(walk)
    same(first, live(cap.run(seeds_d, rs)))
    same(first, live(cap.run(seeds_d, rs)))       # a replay over buffers the previous replay left behind
    other = [[r + 1000 for r in row] for row in rs]
    cap.run(seeds_d, other)
    same(first, live(cap.run(seeds_d, rs)))


for name in sys.argv[2:]:
    globals()["case_" + name]()
    torch.cuda.synchronize()
print("BATCH_RANKS_OK")
"""


def _run(cases, env=None):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _WORKER, root] + list(cases), env=dict(os.environ, **(env or {})), capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0 and "BATCH_RANKS_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


def test_short_batches_three_hops_and_the_products_shape_equal_the_oracle(hiplib):
    """G = 9, B = 7, [5, 5] (batches far shorter than a word); G = 3, B = 200, [15, 10, 5] int64 (three hops, unaligned parts);
    G = 6, B = 256, [25, 10] in int32 / int64 with and without the 32-bit columns.  Every batch equals the oracle and the call
    without the promise gives identical tensors."""
    _run(["short_batches", "three_hops", "products_shape"])


@pytest.mark.parametrize("keys_target", ["100000000", "20000"])
def test_split_and_multi_trip_ranges_count_each_new_vertex_once(hiplib, keys_target):
    """One hash range per batch (it overfills the LDS table, is split and redone, and is longer than one trip), and ranges of
    which some overfill: the per-batch counts of new vertices must not see a neighbour twice."""
    _run(["products_shape"], {"WGAMD_RENUMBER_KEYS_TARGET": keys_target})


def test_a_batch_without_edges_and_a_batch_of_one_hubs_neighbours(hiplib):
    """A batch whose seeds all have degree 0 adds zero new vertices between two live batches; a batch seeded with one hub's
    neighbours is mostly repeats whose first position lies in an earlier part of the batch."""
    _run(["empty_and_hub"])


def test_pyg_walk_uniform_and_uneven_seed_lists(hiplib):
    """PygNoSyncWalk makes the promise only for its own uniform segments: that call, the same segments passed explicitly
    (no promise: today's path) and an uneven seed_seg all equal the oracle, the first two tensor for tensor (frontier lists,
    local ids and segment arrays included)."""
    _run(["pyg"])


def test_a_window_larger_than_lds_keeps_the_plain_path(hiplib):
    """A hop whose per-batch capacity needs more than the 65,536-byte window (352,768 edges: 66,156 bytes) runs as before;
    the result is the oracle's."""
    _run(["window_too_large"])


def test_two_runs_and_a_captured_replay_are_identical(hiplib):
    """Two runs on the same inputs and replays through CapturedWalk give identical tensors: the per-batch counters are cleared
    by the launch chain (the bucketing kernel), not by a memset outside it."""
    _run(["replay"])
