"""GPU: the two small kernels of the temporal heterogeneous call groups, through their C entries.

* ``wgamd_reach_time_append`` (csrc/wg_reach_time.hip) against torch: per batch the old list's times, then the times of the
  vertices the call gained — G in {1, 3}, per-batch (old, new) sizes (0, 0), (0, k), (k, 0), (k, j) with k at 255, 256, 257 (one
  block, exactly one block, one entry into the next); nothing is written past the live total.
* ``graph_ops.rows_first_values`` (``wgamd_rows_first_values``, csrc/wg_rows_unique.hip) against ``link_loader._first_occurrence``
  row by row — S in {1, 2, 63, 64, 65, 257, 8192} (a wave, the 256-position pass and the domain's bound), G in {1, 5}, rows all
  equal, all distinct and random, values negative and near +-2^62, copied exactly; the tail is zero."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = -(1 << 60) - 12345


def _append(time_in, node_seg, f_time, f_seg, out_batch, out_seg, G, cap):
    import torch
    from wholegraph_amd import _lib as L
    from wholegraph_amd.env import get_stream
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()  # noqa: E731
    t_in, t_f = dev(time_in, np.int64), dev(f_time, np.int64)
    segs = [dev(a, np.int32) for a in (node_seg, f_seg, out_batch, out_seg)]
    out = torch.full((cap,), SENTINEL, dtype=torch.int64, device="cuda")
    L.check(L.lib().wgamd_reach_time_append(t_in.data_ptr(), int(t_in.shape[0]), segs[0].data_ptr(), t_f.data_ptr(), int(t_f.shape[0]),
                                            segs[1].data_ptr(), segs[2].data_ptr(), segs[3].data_ptr(), G, cap, out.data_ptr(),
                                            get_stream()), "wgamd_reach_time_append")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _append_case(sizes, rng):
    """``sizes``: per batch (old, new).  Runs the kernel and compares with the per-batch concatenation."""
    G = len(sizes)
    old, new = np.array([s[0] for s in sizes]), np.array([s[1] for s in sizes])
    node_seg = np.concatenate([[0], np.cumsum(old)])
    f_seg = np.concatenate([[0], np.cumsum(new)])
    out_seg = np.concatenate([[0], np.cumsum(old + new)])
    # (both source lists are padded, as the walk's capacity-sized buffers are; the padding must never be read)
    time_in = np.concatenate([rng.integers(-(1 << 62), 1 << 62, node_seg[-1]), np.full(3, 777)]).astype(np.int64)
    f_time = np.concatenate([rng.integers(-(1 << 62), 1 << 62, f_seg[-1]), np.full(3, 888)]).astype(np.int64)
    total = int(out_seg[-1])
    cap = total + 5
    out_batch = np.concatenate([np.repeat(np.arange(G), old + new), np.full(5, 0)])
    got = _append(time_in, node_seg, f_time, f_seg, out_batch, out_seg, G, cap)
    want = np.concatenate([np.concatenate([time_in[node_seg[b]:node_seg[b + 1]], f_time[f_seg[b]:f_seg[b + 1]]]) for b in range(G)]
                          + [np.full(5, SENTINEL)]).astype(np.int64)
    assert np.array_equal(got, want), sizes


@pytest.mark.parametrize("k", [255, 256, 257])
def test_reach_time_append_against_torch(hiplib, k):
    rng = np.random.default_rng(k)
    for sizes in ([(0, 0)], [(0, k)], [(k, 0)], [(k, 7)], [(k, k + 1)]):                       # G = 1
        _append_case(sizes, rng)
    for sizes in ([(0, 0), (0, k), (k, 0)], [(k, 7), (0, 0), (k, k + 1)], [(k, 0), (k, 3), (0, 0)], [(0, k), (5, k), (k, 1)]):   # G = 3
        _append_case(sizes, rng)


def _rows(kind, G, S, n_ids, rng):
    if kind == "equal":
        return np.repeat(rng.integers(0, n_ids, (G, 1)), S, axis=1)
    if kind == "distinct":
        return np.stack([rng.permutation(n_ids)[:S] for _ in range(G)])
    return rng.integers(0, max(S // 3, 2), (G, S))


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 257, 8192])
def test_rows_first_values_against_first_occurrence(hiplib, S):
    import torch
    from cugraph_pyg_amd.loader.link_loader import _first_occurrence
    from wholegraph_amd import graph_ops
    rng = np.random.default_rng(S)
    n_ids = max(2 * S, 4)
    cases = [np.concatenate([_rows("equal", 1, S, n_ids, rng), _rows("distinct", 1, S, n_ids, rng), _rows("random", 3, S, n_ids, rng)])]
    cases += [_rows(kind, 1, S, n_ids, rng) for kind in ("equal", "distinct", "random")]
    for ends in cases:
        G = ends.shape[0]
        values = rng.integers(-(1 << 62), 1 << 62, (G, S)).astype(np.int64)
        values[:, ::3] = -values[:, ::3].clip(min=1)                   # negative values
        values[0, 0], values[-1, -1] = (1 << 62) + 5, -(1 << 62) - 5   # near +-2^62
        e, v = torch.from_numpy(ends.astype(np.int64)).cuda(), torch.from_numpy(values).cuda()
        uniq, seg, batch, local = graph_ops.rows_first_unique(e, n_ids)
        got = graph_ops.rows_first_values(local, seg, v)
        assert got.dtype == torch.int64 and got.shape == (G * S,)
        seg_h = seg.tolist()
        for g in range(G):
            n = seg_h[g + 1] - seg_h[g]
            want = _first_occurrence(local[g], v[g], n)
            assert torch.equal(got[seg_h[g]:seg_h[g + 1]], want), (G, S, g)
        assert not bool(got[seg_h[G]:].any()), "the tail is zero"
